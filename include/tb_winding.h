/* tb_winding.h -- the generalized winding number of a triangle set at a point, the rule stated once for the host (tb_host_scene_winding: brute
 * force and walk; tb_winding_numbers with TB_WINDING_HOST_WALK) and the device (wn_kernels.hip: tb_winding_numbers, tb_bake_winding_field and the sign
 * passes of tb_nearest_points_winding, tb_bake_distance_field_winding).  DESIGN.md section 28.  Built from tb_vec.h / tb_math.h operations only, so
 * every product and sum rounds as those functions state (-ffp-contract=off; tb3_dot is the one fused chain: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)))
 * and host and device give the same bits.
 *
 * w(p) = (sum over the triangles t of Omega_t(p)) * (1 / (4 pi) as a float): inside a closed mesh whose face vectors (tb_normals.h) point outward it
 * is 1, outside 0; inward-facing: -1; two shells: 2; an open mesh, a soup, duplicated triangles: whatever the sum gives, a function of the triangle
 * SET and the point off the surface.
 *
 * tb_solid_angle(p, v0, v1, v2) (Van Oosterom and Strackee 1983), the signed solid angle of one triangle seen from p:
 *   a = v0 - p, b = v1 - p, c = v2 - p;   la = tb_sqrt(tb3_dot(a, a)), lb, lc likewise
 *   num = tb3_dot(a, tb3_cross(b, c))
 *   den = ((la * lb) * lc + tb3_dot(a, b) * lc) + (tb3_dot(b, c) * la + tb3_dot(c, a) * lb)      (every product and sum rounded, none fused)
 *   Omega = 2.0f * tb_atan2(num, den)
 *   Positive where tb_face_vector(v0, v1, v2) points away from p.  tb_atan2(0, 0) = 0: a point on a corner, and a triangle collapsed to a point,
 *   contribute 0.  A point ON the surface gets what the formula gives: deterministic, not meaningful.
 *
 * The exact form: Omega_t summed in one fp32 accumulator in a stated order, then multiplied once by TB_WINDING_INV_4PI.
 *
 * Moments of a subtree (arithmetic, not method -- the same kind of contract as the boxes of a refit):
 *   leaf     A = tb_face_vector(v0, v1, v2) * 0.5f;  area = tb_sqrt(tb3_dot(A, A));  centre = ((v0 + v1) + v2) * TB_WINDING_THIRD;
 *            radius = tb_max(tb_max(|v0 - centre|, |v1 - centre|), |v2 - centre|), |x| = tb_sqrt(tb3_dot(x, x));  N = A
 *   parent   from its children's STORED values, left l and right r:  N = N_l + N_r;  area = area_l + area_r;
 *            centre = area > 0 ? (c_l * area_l + c_r * area_r) / area : (c_l + c_r) * 0.5f       (per component: two products, a sum, a quotient)
 *            radius = tb_max(|centre - c_l| + r_l, |centre - c_r| + r_r)
 *   A parent reads nothing but its two children, so the order in which the nodes of one height are fitted cannot change a bit.
 *
 * The far-field rule (Barill et al. 2018, order 0).  A child with moments (N, c, r) is ACCEPTED iff L2 > (beta * r) * (beta * r), d = c - p,
 * L2 = tb3_dot(d, d), and then contributes tb3_dot(N, d) / (L2 * tb_sqrt(L2)) in place of everything below it -- 0 where that denominator has
 * underflowed to 0 (a subtree of radius < |d| / beta seen from nearer than about 10^-15: |N| <= r^2, so what is dropped is below 1 / beta^2, and
 * 0 / 0 would be a NaN for triangles collapsed to a point); a leaf may be accepted too.  A child
 * that is not accepted contributes tb_solid_angle if it is a leaf and is descended if it is inner.  beta = +inf accepts nothing (inf * 0 is a NaN and
 * the comparison false): the exact form over the tree's order.
 *
 * The order.  One fp32 accumulator per point.  The root's own moments are tested first (a point 10^6 extents away costs one dipole); below it the
 * contributions are added in the order of a depth-first walk that finishes a node's left child, and everything below it, before its right child.
 * So w is a function of (tree topology, triangles, point, beta): not of node numbering, lane or schedule.
 *
 * tb_winding_inside(w) = tb_abs(w) >= 0.5f: agnostic of orientation; a NaN is not inside.  A position with a coordinate that is not finite gives
 * w = TB_WINDING_NAN (0x7fc00000). */
#ifndef TB_WINDING_H
#define TB_WINDING_H

#include "tb_normals.h"

#define TB_WINDING_INV_4PI 0.079577471545947673f
#define TB_WINDING_THIRD 0.333333343267440796f
#define TB_WINDING_NAN 0x7fc00000u

struct TbMoments { tb3 N, c; float r, area; };

TB_HD float tb_solid_angle(tb3 p, tb3 v0, tb3 v1, tb3 v2)
{
    const tb3 a = v0 - p, b = v1 - p, c = v2 - p;
    const float la = tb_sqrt(tb3_dot(a, a)), lb = tb_sqrt(tb3_dot(b, b)), lc = tb_sqrt(tb3_dot(c, c));
    const float num = tb3_dot(a, tb3_cross(b, c));
    const float den = ((la * lb) * lc + tb3_dot(a, b) * lc) + (tb3_dot(b, c) * la + tb3_dot(c, a) * lb);
    return 2.0f * tb_atan2(num, den);
}

TB_HD TbMoments tb_moments_leaf(tb3 v0, tb3 v1, tb3 v2)
{
    TbMoments m;
    m.N = tb_face_vector(v0, v1, v2) * 0.5f;
    m.area = tb_sqrt(tb3_dot(m.N, m.N));
    m.c = ((v0 + v1) + v2) * TB_WINDING_THIRD;
    m.r = tb_max(tb_max(tb3_length(v0 - m.c), tb3_length(v1 - m.c)), tb3_length(v2 - m.c));
    return m;
}

TB_HD TbMoments tb_moments_parent(TbMoments l, TbMoments r)
{
    TbMoments m;
    m.N = l.N + r.N;
    m.area = l.area + r.area;
    m.c = m.area > 0.0f ? (l.c * l.area + r.c * r.area) / m.area : (l.c + r.c) * 0.5f;
    m.r = tb_max(tb3_length(m.c - l.c) + l.r, tb3_length(m.c - r.c) + r.r);
    return m;
}

TB_HD bool tb_winding_accepts(float L2, float r, float beta) { const float br = beta * r; return L2 > br * br; }
TB_HD float tb_winding_dipole(tb3 N, tb3 d, float L2) { const float den = L2 * tb_sqrt(L2); return den > 0.0f ? tb3_dot(N, d) / den : 0.0f; }
TB_HD bool tb_winding_inside(float w) { return tb_abs(w) >= 0.5f; }
TB_HD bool tb_winding_finite3(tb3 p) { return tb_abs(p.x) < tb_u2f(0x7f800000u) && tb_abs(p.y) < tb_u2f(0x7f800000u) && tb_abs(p.z) < tb_u2f(0x7f800000u); }

#endif /* TB_WINDING_H */
