/* rq_launch.h -- the launchers of rq_kernels.hip: ray queries on device buffers (include/tracerboy_hip.h tb_trace_rays).
 *   rq_launch_closest   one ray per lane through the renderer's closest-hit walks; writes hit records, or -- hits null -- one byte per ray: the
 *                       closest hit lies inside the ray's range (two-level scenes in occluded mode; the other side of the measurements)
 *   rq_launch_occluded  the any-hit walk of one-level scenes: one ray per lane (refillMin = 0), or a persistent grid whose waves draw ray indices
 *                       whenever refillMin of their lanes are idle, from pools they claim from *counter
 * Every pointer is a device pointer, rays and hits 16-B aligned.  n <= 2^31.  The stacks are sized as pt_launch_trace_closest sizes them, and a launch
 * is refused where that launcher refuses.  The launchers know neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"

/* Chosen by measurement (scripts/ray_query_rate.py).  RQ_REFILL_MIN: idle lanes at which a wave draws new rays (16 and 32 give
 * the same rate within 2 %, 64 loses up to half of it).  RQ_CHUNK: ray indices a wave claims from the counter with one atomic add.
 * RQ_REFILL_TRIANGLES: the scene size from which the refilling form runs.  It delivers 6.5 to 12 Grays/s on scenes of 2 k to 200 k triangles
 * almost whatever the rays' order; one ray per lane delivers 29 down to 12 Grays/s on camera rays and 8.5 down to 3.5 on shuffled AO rays.  On AO
 * rays in the order of their camera hits the two cross between 10 k (9.8 against 9.3) and 50 k triangles (6.3 against 7.6). */
#define RQ_REFILL_MIN 32u
#define RQ_CHUNK 256u
#define RQ_REFILL_TRIANGLES 32768u
/* refillMin of rq_launch_occluded for a scene of that many triangles */
static inline uint32_t rq_refill_for(uint32_t numTris) { return numTris >= RQ_REFILL_TRIANGLES ? RQ_REFILL_MIN : 0u; }

extern "C" {
hipError_t rq_launch_closest(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const TbQueryRay* rays, TbQueryHit* hits, uint8_t* occluded);
/* refillMin: 0, one ray per lane (counter is not used); 1 .. 64, the refilling form -- counter: one word, zeroed here on the stream */
hipError_t rq_launch_occluded(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const TbQueryRay* rays, uint8_t* occluded, uint32_t* counter,
                              uint32_t refillMin);
}
