/* radiance_trace.h -- what context_radiance.cpp shares with context_bake.cpp: the launch of a radiance query on device buffers. */
#pragma once
#include "context_internal.h"
#include "../kernels/rad_launch.h"

namespace tbctx {
/* context_radiance.cpp: the query k on n device rays into n device sums, planned as tb_trace_radiance plans it, on the context's stream, waited
 * for; TB_OK, or a refusal recorded with fail().  The caller has checked the scene, the settings and the pointers. */
int traceRadianceOnDevice(tb_context* c, const char* who, const tb_output_settings& s, float time, const RadCall& k, uint64_t n, const TbRadianceRay* rays,
    TbFloat4* out);
}
