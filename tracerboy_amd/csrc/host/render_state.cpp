/* render_state.cpp -- render states (include/tracerboy_hip.h tb_state_*): the file format with its host-only readers and
 * writer, and the context's side: begin an accumulation at a frame, save, load (replace) and merge (add).  The reference has no counterpart
 * (its accumulation lives and dies with the process); what is kept from it is the meaning of the surfaces -- sum of rgb * w and of w per pixel,
 * frame index = seed -- which is all a resumed render needs to continue with the same bits.
 * The device work is two streaming kernels (kernels/state_kernels.hip): the digest of the surfaces and dst += src. */
#include "context_internal.h"
#include "../kernels/state_launch.h"
#include "tb_state.h"

#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>

using namespace tbhost;
using namespace tbctx;

static_assert(sizeof(tb_state_info) == 208, "tb_state_info is part of the file format");
static_assert(sizeof(tb_state_info) + 8 <= TB_STATE_HEADER_BYTES, "the header holds the magic and tb_state_info");

namespace {

const char kMagic[8] = {'T', 'B', 'S', 'T', 'A', 'T', 'E', '1'};
const uint32_t kMaxSide = 16384; /* beginCall's limit (context_render.cpp) */

struct File { FILE* f = nullptr; ~File() { if (f) fclose(f); } };

uint64_t surfaceBytes(const tb_state_info& h) { return (uint64_t)h.width * h.height * sizeof(TbFloat4); }
uint64_t hostDigest(const void* words, uint64_t nWords) { TbStateDigest d{0, 0}; tb_state_digest_words(&d, (const uint32_t*)words, nWords); return d.sum; }

/* the fields a reader relies on before it sizes anything; "" = fine */
std::string invalidField(const tb_state_info& h)
{
    if (h.width == 0 || h.height == 0 || h.width > kMaxSide || h.height > kMaxSide) return "width / height: a frame has 1 to 16384 pixels a side";
    if (h.first_frame > h.next_frame) return "first_frame is past next_frame";
    if (h.tile_world == 0 || h.tile_rank >= h.tile_world || h.tile_w == 0 || h.tile_h == 0) return "tile assignment (rank, world, tile size)";
    if (h.tile_world > 1 && (h.tile_w % 16 || h.tile_h % 16)) return "tile assignment: tile width and height are multiples of 16";
    if (h.adaptive_min_frames < 0 || h.adaptive_test > 1) return "adaptive_min_frames / adaptive_test";
    return "";
}

/* open, read and validate the header, compare the file's length with what the header promises; leaves the file at the first surface */
int openState(const char* path, File& file, tb_state_info& h, std::string& err)
{
    if (!path) { err = "null path"; return TB_E_INVALID; }
    file.f = fopen(path, "rb");
    if (!file.f) { err = std::string("cannot open state file ") + path; return TB_E_IO; }
    uint8_t header[TB_STATE_HEADER_BYTES];
    if (fread(header, 1, sizeof header, file.f) != sizeof header) { err = std::string(path) + ": truncated: shorter than a state file's header"; return TB_E_PARSE; }
    if (memcmp(header, kMagic, 8) != 0) { err = std::string(path) + ": bad magic: not a render-state file"; return TB_E_PARSE; }
    memcpy(&h, header + 8, sizeof h);
    if (h.version != TB_STATE_VERSION) { err = std::string(path) + ": version " + std::to_string(h.version) + " (this library reads version " +
        std::to_string(TB_STATE_VERSION) + ")"; return TB_E_PARSE; }
    const std::string bad = invalidField(h);
    if (!bad.empty()) { err = std::string(path) + ": malformed header: " + bad; return TB_E_PARSE; }
    struct stat st;
    if (fstat(fileno(file.f), &st) != 0) { err = std::string("cannot open state file ") + path + " (fstat)"; return TB_E_IO; }
    const uint64_t want = (uint64_t)TB_STATE_HEADER_BYTES + 2u * surfaceBytes(h);
    if ((uint64_t)st.st_size != want) { err = std::string(path) + ": " + ((uint64_t)st.st_size < want ? "truncated" : "too long") + ": " +
        std::to_string((uint64_t)st.st_size) + " bytes, the header promises " + std::to_string(want); return TB_E_PARSE; }
    return TB_OK;
}

/* the surfaces behind an opened header, checked against the stored digests */
int readSurfaces(const char* path, File& file, const tb_state_info& h, float* output, float* jittered, std::string& err)
{
    const uint64_t bytes = surfaceBytes(h);
    float* dst[2] = {output, jittered}; const uint64_t want[2] = {h.output_digest, h.jittered_digest}; const char* name[2] = {"output", "jittered"};
    std::vector<float> spare;
    for (int k = 0; k < 2; k++) {
        float* p = dst[k];
        if (!p) { spare.resize((size_t)(bytes / 4)); p = spare.data(); }
        if (fread(p, 1, (size_t)bytes, file.f) != (size_t)bytes) { err = std::string(path) + ": truncated " + name[k] + " surface"; return TB_E_PARSE; }
        if (hostDigest(p, bytes / 4) != want[k]) { err = std::string(path) + ": " + name[k] + "_digest mismatch: the surface is not what was saved";
            return TB_E_PARSE; }
    }
    return TB_OK;
}

/* header + surfaces beside `path`, then renamed over it: a reader sees the old file or the new one, never a part */
int writeState(const char* path, const tb_state_info& h, const float* output, const float* jittered, std::string& err)
{
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long long)getpid());
    uint8_t header[TB_STATE_HEADER_BYTES]; memset(header, 0, sizeof header);
    memcpy(header, kMagic, 8); memcpy(header + 8, &h, sizeof h);
    const size_t bytes = (size_t)surfaceBytes(h);
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot open " + tmp + " for writing"; return TB_E_IO; }
    bool ok = fwrite(header, 1, sizeof header, f) == sizeof header && fwrite(output, 1, bytes, f) == bytes && fwrite(jittered, 1, bytes, f) == bytes;
    ok = fflush(f) == 0 && ok; ok = fsync(fileno(f)) == 0 && ok; ok = fclose(f) == 0 && ok;
    if (ok && rename(tmp.c_str(), path) != 0) ok = false;
    if (!ok) { (void)unlink(tmp.c_str()); err = std::string("cannot write state file ") + path; return TB_E_IO; }
    return TB_OK;
}

int hostFail(char* err, uint32_t n, int code, const std::string& m) { if (err && n) { strncpy(err, m.c_str(), n - 1); err[n - 1] = 0; } return code; }

/* ---- the context's side ---- */
bool sameBits(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
bool sameTiles(const TbTileMap& t, const tb_state_info& h) { return t.rank == h.tile_rank && t.world == h.tile_world && t.tileW == h.tile_w && t.tileH == h.tile_h; }

uint64_t sceneDigestCached(tb_context* c)
{
    const uint64_t key = ((uint64_t)c->sceneGeneration << 32) | c->materialEdits;
    if (c->sceneDigestKey != key) { refreshHostScene(c); c->sceneDigest = sceneDigestOf(c->scene); c->sceneDigestKey = key; }
    return c->sceneDigest;
}

/* digests of two surfaces of nWords words each, on x's device and stream; waits */
void deviceDigest(tb_context* x, const void* a, const void* b, uint64_t nWords, uint64_t out[2])
{
    ensure(x->stateScratch, (size_t)TB_STATE_DIGEST_SCRATCH_WORDS * 8u);
    uint64_t* scratch = (uint64_t*)x->stateScratch.p;
    HIP_TRY(hipEventRecord(x->evState[0].create(), x->stream));
    HIP_TRY(state_launch_digest(x->stream, (const uint32_t*)a, (const uint32_t*)b, nWords, scratch));
    HIP_TRY(hipEventRecord(x->evState[1].create(), x->stream));
    HIP_TRY(hipMemcpyAsync(out, scratch + 2u * TB_STATE_DIGEST_MAX_GROUPS, 16, hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    if (hipEventElapsedTime(&x->lastStateDigestMs, x->evState[0], x->evState[1]) != hipSuccess) x->lastStateDigestMs = 0.0f;
}

/* x holds the frames [first, next) of a W x H accumulation under these settings: surfaces sized (contents are the caller's), AOVs released as on a
 * resize, the counters a render clears at frame 0 cleared -- a render that starts past frame 0 adds to what it finds */
void adopt(tb_context* x, uint32_t W, uint32_t H, const tb_output_settings& s, float timeSeed, uint32_t first, uint32_t next)
{
    const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
    ensure(x->output, bytes); ensure(x->jittered, bytes);
    for (DevBuf& b : x->aov) b.release();
    ensure(x->stats, 16); HIP_TRY(hipMemsetAsync(x->stats.p, 0, 16, x->stream));
    if (opt<OPT_count_rays>(x) || opt<OPT_debug_profile_groups>(x)) ensure(x->rayStats, 21 * 8);
    if (x->rayStats.p) HIP_TRY(hipMemsetAsync(x->rayStats.p, 0, x->rayStats.bytes, x->stream));
    x->width = W; x->height = H; x->lastSettings = s; x->haveLastSettings = true; x->lastTime = timeSeed;
    x->firstFrame = first; x->samplesRendered = next; x->rt.lastRender = false;
    touchAccumulation(x); x->dn.aovStaleUntilCall = x->callCount + 1; /* the state's frames come without AOVs (context_denoise.cpp) */
}

/* a group deals 64x64 tiles round-robin (renderGroup): with the map in place already the group's first render keeps the frames */
void setGroupTiles(const std::vector<tb_context*>& all)
{
    if (all.size() < 2) return;
    for (uint32_t i = 0; i < (uint32_t)all.size(); i++) all[i]->tiles = TbTileMap{i, (uint32_t)all.size(), 64, 64};
}

} // namespace

extern "C" {

uint64_t tb_state_digest_host(const void* words, uint64_t nWords) { return words ? hostDigest(words, nWords) : 0; }

int tb_state_info_read(const char* path, tb_state_info* out, char* err, uint32_t errLen)
{
    if (!out) return TB_E_INVALID;
    try {
        File file; std::string m; tb_state_info h;
        const int rc = openState(path, file, h, m);
        if (rc != TB_OK) return hostFail(err, errLen, rc, m);
        *out = h; return TB_OK;
    } catch (const std::exception& e) { return hostFail(err, errLen, TB_E_IO, e.what()); }
}

int tb_state_read_host(const char* path, tb_state_info* out, float* output, float* jittered, char* err, uint32_t errLen)
{
    if (!out) return TB_E_INVALID;
    try {
        File file; std::string m; tb_state_info h;
        int rc = openState(path, file, h, m);
        if (rc == TB_OK) rc = readSurfaces(path, file, h, output, jittered, m);
        if (rc != TB_OK) return hostFail(err, errLen, rc, m);
        *out = h; return TB_OK;
    } catch (const std::exception& e) { return hostFail(err, errLen, TB_E_IO, e.what()); }
}

int tb_state_write_host(const char* path, const tb_state_info* in, const float* output, const float* jittered)
{
    if (!path || !in || !output || !jittered) return TB_E_INVALID;
    try {
        tb_state_info h = *in; h.version = TB_STATE_VERSION;
        if (!invalidField(h).empty()) return TB_E_INVALID;
        const uint64_t words = surfaceBytes(h) / 4;
        h.output_digest = hostDigest(output, words); h.jittered_digest = hostDigest(jittered, words);
        std::string m;
        return writeState(path, h, output, jittered, m);
    } catch (const std::exception&) { return TB_E_IO; }
}

int tb_scene_digest(tb_context* c, uint64_t* out)
{
    if (!c || !out) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "tb_scene_digest: no scene loaded");
    *out = sceneDigestCached(c);
    return TB_OK;
}

int tb_accum_digest(tb_context* c, uint64_t out2[2])
{
    return guarded(c, [&]() {
        if (!out2 || !c->output.p || !c->width) return fail(c, TB_E_INVALID, "tb_accum_digest: nothing rendered yet");
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        deviceDigest(c, c->output.p, c->jittered.p, (uint64_t)c->width * c->height * 4u, out2);
        return TB_OK;
    });
}

int tb_state_begin(tb_context* c, uint32_t W, uint32_t H, const tb_output_settings* settings, float timeSeed, uint32_t firstFrame)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (W == 0 || H == 0 || W > kMaxSide || H > kMaxSide) return fail(c, TB_E_INVALID, "tb_state_begin: width / height: a frame has 1 to 16384 pixels a side");
        tb_output_settings s; if (settings) s = *settings; else DefaultOutputSettings(s);
        const std::vector<tb_context*> all = members(c);
        setGroupTiles(all);
        for (tb_context* x : all) {
            DeviceScope scope(x->device);
            HIP_TRY(hipStreamSynchronize(x->stream));
            adopt(x, W, H, s, timeSeed, firstFrame, firstFrame);
            /* the kernels overwrite the surfaces at global frame 0 only: an accumulation that starts later starts from zeros */
            HIP_TRY(hipMemsetAsync(x->output.p, 0, x->output.bytes, x->stream)); HIP_TRY(hipMemsetAsync(x->jittered.p, 0, x->jittered.bytes, x->stream));
        }
        return TB_OK;
    });
}

int tb_state_save(tb_context* c, const char* path)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!path) return fail(c, TB_E_INVALID, "tb_state_save: null path");
        if (c->rt.lastRender) return fail(c, TB_E_INVALID, "tb_state_save: the last render was tb_render_realtime: its surface holds one frame, not an accumulation");
        if (!c->output.p || !c->width || !c->haveLastSettings || c->samplesRendered == c->firstFrame) return fail(c, TB_E_INVALID,
            "tb_state_save: nothing rendered: the context holds no frames");
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        tb_state_info h; memset(&h, 0, sizeof h);
        h.version = TB_STATE_VERSION; h.width = c->width; h.height = c->height; h.first_frame = c->firstFrame; h.next_frame = c->samplesRendered;
        h.time_seed = c->lastTime; h.settings = c->lastSettings; h.camera = c->camera;
        const TbTileMap tiles = c->group.peers.empty() ? c->tiles : TbTileMap{0, 1, 64, 64}; /* a group's context holds the assembled frame */
        h.tile_rank = tiles.rank; h.tile_world = tiles.world; h.tile_w = tiles.tileW; h.tile_h = tiles.tileH;
        h.alpha_test = opt<OPT_alpha_test>(c) ? 1u : 0u; h.adaptive = opt<OPT_adaptive>(c) ? 1u : 0u; h.adaptive_test = (uint32_t)opt<OPT_adaptive_test>(c);
        h.adaptive_min_frames = opt<OPT_adaptive_min_frames>(c);
        h.scene_digest = c->hasScene ? sceneDigestCached(c) : 0;
        const uint64_t words = (uint64_t)c->width * c->height * 4u;
        uint64_t dev[2];
        deviceDigest(c, c->output.p, c->jittered.p, words, dev); /* of the surfaces as they lie in HBM */
        h.output_digest = dev[0]; h.jittered_digest = dev[1];
        std::vector<float> out((size_t)words), jit((size_t)words);
        HIP_TRY(hipMemcpy(out.data(), c->output.p, (size_t)words * 4u, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(jit.data(), c->jittered.p, (size_t)words * 4u, hipMemcpyDeviceToHost));
        if (hostDigest(out.data(), words) != dev[0] || hostDigest(jit.data(), words) != dev[1]) return fail(c, TB_E_DEVICE,
            "tb_state_save: the copied surfaces do not have the digests the device computed (output_digest / jittered_digest)");
        std::string m;
        const int rc = writeState(path, h, out.data(), jit.data(), m);
        return rc == TB_OK ? TB_OK : fail(c, rc, "tb_state_save: " + m);
    });
}

int tb_state_load(tb_context* c, const char* path, uint32_t flags)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (flags & ~(uint32_t)(TB_STATE_ADD | TB_STATE_ANY_SCENE)) return fail(c, TB_E_INVALID, "tb_state_load: unknown flag");
        const bool add = (flags & TB_STATE_ADD) != 0;
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "tb_state_load: no scene loaded");
        /* everything that can refuse the file comes before the first allocation or copy */
        File file; std::string m; tb_state_info h;
        int rc = openState(path, file, h, m);
        if (rc != TB_OK) return fail(c, rc, "tb_state_load: " + m);
        if (!(flags & TB_STATE_ANY_SCENE) && h.scene_digest != sceneDigestCached(c)) return fail(c, TB_E_INVALID,
            "tb_state_load: scene_digest: the state was rendered of another scene (other file, BVH builder or material edit; TB_STATE_ANY_SCENE overrides)");
        const bool ctxComplete = !c->group.peers.empty() || c->tiles.world == 1, fileComplete = h.tile_world == 1;
        const bool sameAssignment = c->group.peers.empty() && sameTiles(c->tiles, h);
        if (add) {
            if (!c->output.p || !c->width || !c->haveLastSettings) return fail(c, TB_E_INVALID, "tb_state_load: TB_STATE_ADD needs a context that holds a state");
            if (c->rt.lastRender) return fail(c, TB_E_INVALID, "tb_state_load: TB_STATE_ADD after tb_render_realtime: the surface holds no accumulation");
            if (h.width != c->width || h.height != c->height) return fail(c, TB_E_INVALID, "tb_state_load: width / height differ from the context's");
            if (historyRelevantChange(h.settings, c->lastSettings)) return fail(c, TB_E_INVALID, "tb_state_load: settings differ from the context's in a history-relevant member");
            if (!sameBits(&h.time_seed, &c->lastTime, 4)) return fail(c, TB_E_INVALID, "tb_state_load: time_seed differs from the context's");
            if (!sameBits(&h.camera, &c->camera, sizeof h.camera)) return fail(c, TB_E_INVALID, "tb_state_load: camera differs from the context's");
            if (!((ctxComplete && fileComplete) || sameAssignment)) return fail(c, TB_E_INVALID,
                "tb_state_load: tile assignment: a complete frame adds to a complete frame, a rank's part to the same rank's part");
            if (h.first_frame != c->samplesRendered && h.next_frame != c->firstFrame) return fail(c, TB_E_INVALID,
                "tb_state_load: first_frame / next_frame: the file's frames [" + std::to_string(h.first_frame) + ", " + std::to_string(h.next_frame) +
                ") neither follow nor precede the context's [" + std::to_string(c->firstFrame) + ", " + std::to_string(c->samplesRendered) + "): overlap or gap");
        } else {
            if (!(fileComplete || sameAssignment)) return fail(c, TB_E_INVALID,
                "tb_state_load: tile assignment: a rank's partial frame loads only into a context with the same tb_set_tile_assignment");
            if (h.alpha_test != (opt<OPT_alpha_test>(c) ? 1u : 0u)) return fail(c, TB_E_INVALID, "tb_state_load: option alpha_test differs from the file's");
            if (h.adaptive != (opt<OPT_adaptive>(c) ? 1u : 0u)) return fail(c, TB_E_INVALID, "tb_state_load: option adaptive differs from the file's");
            if (h.adaptive_min_frames != opt<OPT_adaptive_min_frames>(c)) return fail(c, TB_E_INVALID, "tb_state_load: option adaptive_min_frames differs from the file's");
            if ((int64_t)h.adaptive_test != opt<OPT_adaptive_test>(c)) return fail(c, TB_E_INVALID, "tb_state_load: option adaptive_test differs from the file's");
        }
        const uint64_t words = surfaceBytes(h) / 4; const size_t bytes = (size_t)surfaceBytes(h);
        std::vector<float> out((size_t)words), jit((size_t)words);
        rc = readSurfaces(path, file, h, out.data(), jit.data(), m);
        if (rc != TB_OK) return fail(c, rc, "tb_state_load: " + m);

        const std::vector<tb_context*> all = members(c);
        auto forget = [&]() { for (tb_context* x : all) resetHistory(x); };
        for (tb_context* x : all) {
            DeviceScope scope(x->device);
            HIP_TRY(hipStreamSynchronize(x->stream));
            DevBuf fileOut, fileJit; /* the file's copies of an addition: released at the end of the member's turn */
            void *dstOut = nullptr, *dstJit = nullptr;
            if (add) { ensure(fileOut, bytes); ensure(fileJit, bytes); dstOut = fileOut.p; dstJit = fileJit.p; }
            else { adopt(x, h.width, h.height, h.settings, h.time_seed, h.first_frame, h.next_frame); dstOut = x->output.p; dstJit = x->jittered.p; }
            uint64_t dev[2] = {0, 0};
            try {
                HIP_TRY(hipMemcpyAsync(dstOut, out.data(), bytes, hipMemcpyHostToDevice, x->stream));
                HIP_TRY(hipMemcpyAsync(dstJit, jit.data(), bytes, hipMemcpyHostToDevice, x->stream));
                deviceDigest(x, dstOut, dstJit, words, dev); /* HBM -> file -> HBM: the same bits lie on the device again */
            } catch (...) { if (!add) forget(); throw; }
            if (dev[0] != h.output_digest || dev[1] != h.jittered_digest) { if (!add) forget(); return fail(c, TB_E_DEVICE,
                "tb_state_load: output_digest / jittered_digest: the uploaded surfaces do not have the file's digests on device " + std::to_string(x->device)); }
            if (add) {
                touchAccumulation(x); x->dn.aovStaleUntilCall = x->callCount + 1;
                if (x->samplesRendered == x->firstFrame) { /* an empty range: whatever an earlier history left in the surfaces does not count */
                    HIP_TRY(hipMemsetAsync(x->output.p, 0, bytes, x->stream)); HIP_TRY(hipMemsetAsync(x->jittered.p, 0, bytes, x->stream)); }
                HIP_TRY(hipEventRecord(x->evState[0].create(), x->stream));
                HIP_TRY(state_launch_add(x->stream, (float*)x->output.p, (const float*)dstOut, (float*)x->jittered.p, (const float*)dstJit, words));
                HIP_TRY(hipEventRecord(x->evState[1].create(), x->stream));
                HIP_TRY(hipStreamSynchronize(x->stream)); /* the file's copies are released below */
                if (hipEventElapsedTime(&x->lastStateAddMs, x->evState[0], x->evState[1]) != hipSuccess) x->lastStateAddMs = 0.0f;
            }
        }
        if (add) {
            const bool append = h.first_frame == c->samplesRendered;
            for (tb_context* x : all) { if (append) x->samplesRendered = h.next_frame; else x->firstFrame = h.first_frame; }
        } else {
            setGroupTiles(all);
            for (tb_context* x : all) { /* tb_set_camera without its history reset */
                x->camera = h.camera; x->ds.config.CameraLensHeight = h.camera.LensHeight; x->scene.config.CameraLensHeight = h.camera.LensHeight; }
        }
        return TB_OK;
    });
}

} // extern "C"
