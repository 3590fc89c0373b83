/* tb_nearest.h -- the nearest point of a triangle set to a point, the rule stated once for the host (tb_host_scene_nearest: brute force and walk)
 * and the device (pq_kernels.hip: tb_nearest_points, tb_bake_distance_field).  DESIGN.md section 27.  Built from tb_vec.h operations only, so every
 * product and sum rounds as those functions state (-ffp-contract=off; tb3_dot is the one fused chain: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))) and
 * host and device give the same bits.
 *
 * tb_nearest_on_triangle(p, v0, v1, v2) -> (U, V, Point, D2): the Voronoi-region method (Ericson, Real-Time Collision Detection, section 5.1.5).
 *   ab = v1 - v0, ac = v2 - v0, ap = p - v0, bp = p - v1, cp = p - v2
 *   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
 *   vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4        (two rounded products, one rounded difference each)
 *   The regions, in this order; the first whose condition holds decides (U, V), the weights of v1 and v2:
 *     vertex 0   d1 <= 0 and d2 <= 0                                  (0, 0)
 *     vertex 1   d3 >= 0 and d4 <= d3                                 (1, 0)
 *     vertex 2   d6 >= 0 and d5 <= d6                                 (0, 1)
 *     edge AB    vc <= 0 and d1 >= 0 and d3 <= 0                      (d1 / (d1 - d3), 0)
 *     edge AC    vb <= 0 and d2 >= 0 and d6 <= 0                      (0, d2 / (d2 - d6))
 *     edge BC    va <= 0 and e = d4 - d3 >= 0 and f = d5 - d6 >= 0    w = e / (e + f): (1 - w, w)
 *     interior   a = max(va, 0), b = max(vb, 0), c = max(vc, 0), s = (a + b) + c: (b / s, c / s).  The clamps are this file's: where rounding
 *                has left one of the three negative although no edge region took the point, the weights stay inside [0, 1] and U + V <= 1 up to
 *                the roundings of s and the two quotients.
 *   A quotient whose denominator is 0 is 0 (tb_nearest_quotient), so a triangle that is a segment or a point gives a finite point of itself.
 *   Point = (v0 + ab * U) + ac * V        (two rounded products and two rounded sums per component, none fused)
 *   D2 = dot(p - Point, p - Point)
 *   No NaN leaves the function for finite input whose differences and products stay finite.
 *
 * The candidate rule.  limit = tb_nearest_limit(MaxDistance): the largest float x with tb_sqrt(x) <= MaxDistance -- MaxDistance * MaxDistance
 * rounded once, then moved by at most two floats down or three up until that holds; +inf for +inf; -1 (nothing counts) for a MaxDistance that is a
 * NaN or negative.  A triangle counts iff D2 <= limit, which is to say iff the Distance its record would carry, tb_sqrt(D2), is <= MaxDistance:
 * the plain product alone would turn away a triangle at exactly the distance asked for wherever sqrt rounds down (D2 = 2: tb_sqrt(2)^2 rounds to
 * the float below 2).  Among the triangles that count the smallest D2 wins; equal D2 is settled by the smaller geometryIndex, then the smaller
 * primitiveIndex (tb_nearest_better).  So the answer is a function of the triangle SET and the point: not of the tree, the builder, the order of
 * visits or the schedule.  A query position with a coordinate that is not finite is a miss.
 *
 * tb_box_d2(p, centre, half): q_k = max(|p_k - c_k| - h_k, 0), dot(q, q).
 *
 * The pruning rule.  A subtree is skipped only if the tb_box_d2 of its box is > tb_nearest_cull(bound, E), bound = min(limit, best D2 so far):
 *     cull = ((sqrt(bound) + E) * (sqrt(bound) + E)) * (1 + 2^-20),      E = TB_NEAREST_SLACK_ULPS * 2^-23 * M,
 * M the largest coordinate magnitude among the root box's corners (|c_k| + h_k) and the point (tb_nearest_scale).  The slack is needed: the fp32
 * box of a triangle, as centre and half-extent, can give a tb_box_d2 LARGER than the triangle's own fp32 D2, and the builders' and the refit's
 * boxes carry their own roundings, so `box > best` loses winners.  Measured (scripts/nearest_slack.py: tb_host_scene_nearest_excess over every
 * case of tests/adversarial_cases.py x the host builders 0, 1, 3, 1500 points of tests/nearest_cases.py each, three seeds): the largest
 * sqrt(box d2) - sqrt(D2) over the boxes above a winner, the root's included, is 1.959 x 2^-23 x M (rand257, builder 3, seed 70).  TB_NEAREST_SLACK_ULPS = 16, eight times that.
 * The factor (1 + 2^-20) covers the roundings of the root, the sum, the square and of tb_box_d2's own three squares and two sums.  cull is made
 * again only when the bound improves.  The comparison is >, never >=: cull >= bound, so every triangle that ties with the best survives the prune
 * and the tie-break sees it.
 *
 * Sign (TB_NEAREST_SIGNED).  Distance is negated iff dot(p - Point, tb_face_vector(v0, v1, v2)) < 0 for the winning triangle; on its plane, and
 * for a face vector of zero, it stays positive.  This is the side of the NEAREST TRIANGLE: exact where the nearest point is interior to a
 * triangle; wrong for about one point in twenty near edges or vertices whose faces meet at an acute angle, a regular tetrahedron included; see
 * section 28 (tb_winding.h has the robust sign). */
#ifndef TB_NEAREST_H
#define TB_NEAREST_H

#include "tb_normals.h"

#define TB_NEAREST_SLACK_ULPS 16.0f
#define TB_NEAREST_NONE 0xffffffffu

struct TbNearestOnTriangle { float U, V; tb3 Point; float D2; };

TB_HD float tb_nearest_quotient(float a, float b) { return b == 0.0f ? 0.0f : a / b; }

TB_HD TbNearestOnTriangle tb_nearest_on_triangle(tb3 p, tb3 v0, tb3 v1, tb3 v2)
{
    const tb3 ab = v1 - v0, ac = v2 - v0, ap = p - v0, bp = p - v1, cp = p - v2;
    const float d1 = tb3_dot(ab, ap), d2 = tb3_dot(ac, ap), d3 = tb3_dot(ab, bp), d4 = tb3_dot(ac, bp), d5 = tb3_dot(ab, cp), d6 = tb3_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e = d4 - d3, f = d5 - d6;
    const float a = tb_max(va, 0.0f), b = tb_max(vb, 0.0f), c = tb_max(vc, 0.0f), s = (a + b) + c;
    float U, V;
    if (d1 <= 0.0f && d2 <= 0.0f) { U = 0.0f; V = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { U = 1.0f; V = 0.0f; }
    else if (d6 >= 0.0f && d5 <= d6) { U = 0.0f; V = 1.0f; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { U = tb_nearest_quotient(d1, d1 - d3); V = 0.0f; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { U = 0.0f; V = tb_nearest_quotient(d2, d2 - d6); }
    else if (va <= 0.0f && e >= 0.0f && f >= 0.0f) { V = tb_nearest_quotient(e, e + f); U = 1.0f - V; }
    else { U = tb_nearest_quotient(b, s); V = tb_nearest_quotient(c, s); }
    TbNearestOnTriangle r;
    r.U = U; r.V = V;
    r.Point = (v0 + ab * U) + ac * V;
    const tb3 d = p - r.Point;
    r.D2 = tb3_dot(d, d);
    return r;
}

/* the largest float x with tb_sqrt(x) <= maxDistance; -1: nothing counts */
TB_HD float tb_nearest_limit(float maxDistance)
{
    if (!(maxDistance >= 0.0f)) return -1.0f;
    const uint32_t inf = 0x7f800000u;
    if (tb_f2u(maxDistance) == inf) return maxDistance;
    uint32_t x = tb_f2u(maxDistance * maxDistance); /* not negative: its bits order as its values do */
    for (int k = 0; k < 2 && x > 0u && (x == inf || tb_sqrt(tb_u2f(x)) > maxDistance); k++) x--;
    for (int k = 0; k < 3 && x + 1u < inf && tb_sqrt(tb_u2f(x + 1u)) <= maxDistance; k++) x++;
    return tb_u2f(x);
}

TB_HD bool tb_nearest_finite3(tb3 p) { return tb_abs(p.x) < tb_u2f(0x7f800000u) && tb_abs(p.y) < tb_u2f(0x7f800000u) && tb_abs(p.z) < tb_u2f(0x7f800000u); }

/* (d2, geom, prim) beats (bestD2, bestGeom, bestPrim); no candidate yet: bestD2 = +inf, bestGeom = bestPrim = TB_NEAREST_NONE */
TB_HD bool tb_nearest_better(float d2, uint32_t geom, uint32_t prim, float bestD2, uint32_t bestGeom, uint32_t bestPrim)
{
    return d2 < bestD2 || (d2 == bestD2 && (geom < bestGeom || (geom == bestGeom && prim < bestPrim)));
}

TB_HD float tb_box_d2(tb3 p, tb3 centre, tb3 half)
{
    const tb3 q = tb3_max(tb3_abs(p - centre) - half, tb3_splat(0.0f));
    return tb3_dot(q, q);
}

TB_HD float tb_nearest_scale(tb3 p, tb3 rootCentre, tb3 rootHalf)
{
    const tb3 m = tb3_max(tb3_abs(rootCentre) + rootHalf, tb3_abs(p));
    return tb_max(tb_max(m.x, m.y), m.z);
}
TB_HD float tb_nearest_slack(float scale) { return (TB_NEAREST_SLACK_ULPS * 1.1920928955078125e-7f) * scale; }
TB_HD float tb_nearest_cull(float bound, float slack)
{
    const float s = tb_sqrt(bound) + slack;
    return (s * s) * 1.00000095367431640625f;
}

TB_HD bool tb_nearest_behind(tb3 p, tb3 point, tb3 v0, tb3 v1, tb3 v2) { return tb3_dot(p - point, tb_face_vector(v0, v1, v2)) < 0.0f; }

#endif /* TB_NEAREST_H */
