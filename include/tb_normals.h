/* tb_normals.h -- smooth shading normals of a triangle mesh, the rule stated once for the host (tb_host_smooth_normals, TB_MESH_NORMALS_SMOOTH) and the
 * device (refit_kernels.hip: tb_recompute_normals).  Built from tb_vec.h operations only, so every product and sum rounds as those functions state
 * (-ffp-contract=off; tb3_dot is the one fused chain) and host and device give the same bits.
 *   face vector of a triangle (i0, i1, i2):  f = cross(p[i2] - p[i0], p[i2] - p[i1]) -- the loader's operands and order for a mesh without normals
 *                                            (host_scene.cpp AppendGeometry), not normalised: its length is twice the area, which is the weight
 *   vertex v:  acc = 0; over the mesh's triangles in ascending primitive index and, inside a triangle, corners 0, 1, 2: acc = acc + f for every corner
 *              that names v (a triangle that names v twice adds twice)
 *   normal:    (0, 1, 0) where dot(acc, acc) <= 0.0000000001f (the loader's threshold and fallback), else tb3_normalize(acc); what is not finite
 *              is stored as it comes
 * A vertex that no triangle names is not written by either side. */
#ifndef TB_NORMALS_H
#define TB_NORMALS_H

#include "tb_vec.h"

TB_HD tb3 tb_face_vector(tb3 p0, tb3 p1, tb3 p2) { return tb3_cross(p2 - p0, p2 - p1); }
TB_HD tb3 tb_normal_accumulate(tb3 acc, tb3 f) { return acc + f; }
TB_HD tb3 tb_normal_finish(tb3 acc)
{
    if (tb3_dot(acc, acc) <= 0.0000000001f) return tb3_make(0.0f, 1.0f, 0.0f);
    return tb3_normalize(acc);
}

#endif /* TB_NORMALS_H */
