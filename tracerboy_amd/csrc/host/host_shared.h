/* host_shared.h -- what host_api.cpp, which knows no device, shares with the context's translation units.  No HIP header. */
#pragma once
#include "host_scene.h"

namespace tbctx {
extern std::string g_createError; /* tb_last_error(nullptr): the last failure of a call that has no context (context.cpp) */
/* host_api.cpp */
void fillSceneInfo(const tbhost::HostScene& s, tb_scene_info* o);
void fillView(const tbhost::HostScene& s, TbSceneView* v);
uint64_t sceneDigestOf(const tbhost::HostScene& s);
} // namespace tbctx
