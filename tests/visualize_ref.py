"""numpy restatement of the ray visualiser's overlay (tracerboy_amd/csrc/kernels/vis_kernels.hip vis_overlay; the reference's
VisualizeRaysCS.hlsl:133-226), one float32 operation per line in the kernel's order: IEEE binary32, unfused,
    dot(a, b) = (ax bx + ay by) + az bz,   normalize(v) = v / sqrt(dot(v, v)),   lerp(a, b, s) = a + s (b - a),
with the divisions by zero the reference has (k2 == 0, bard == 0) left in: their infinities and NaNs fail the comparisons behind them.
Every pixel of the picture is computed at once, (H, W) arrays; the loop over the rays is Python's.  Early returns of the kernel's helpers are
np.where chains here: every side is computed, the kernel's conditions select."""
import numpy as np

F = np.float32
MAX_RAYS = 1024
FAR = F(9999999.9)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def div(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def normalize(a):
    return div(a, np.sqrt(dot(a, a)))


def vec(v):
    return (F(v[0]), F(v[1]), F(v[2]))


def constants(camera, width, height, ray_width=0.01, ray_depth=10.0, ray_count=0):
    """VisualizationRaysConstants as TracerBoy.cpp:3216-3228 fills them; camera: Position, LookAt, Right, Up, LensHeight, FocalDistance."""
    class K:
        pass
    k = K()
    k.ResolutionX, k.ResolutionY = int(width), int(height)
    k.CylinderRadius, k.RayDepth, k.RayCount = F(ray_width), F(ray_depth), int(ray_count) if ray_count > 0 else 999999
    k.FocalLength, k.LensHeight = F(camera.FocalDistance), F(camera.LensHeight)
    k.CameraPosition, k.CameraLookAt, k.CameraRight, k.CameraUp = vec(camera.Position), vec(camera.LookAt), vec(camera.Right), vec(camera.Up)
    k.Padding2 = F(0)
    return k


@np.errstate(all="ignore")
def camera_rays(k):
    """:138-149: the lens position and direction of every pixel's view ray -- no half-pixel offset, uv.y flipped."""
    W, H = int(k.ResolutionX), int(k.ResolutionY)
    res_x, res_y = F(W), F(H)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    u = x / res_x
    v = F(1) - y / res_y
    aspect = res_x / res_y
    pos = vec(k.CameraPosition)
    view = normalize(sub(vec(k.CameraLookAt), pos))
    focal = sub(pos, mul(view, F(k.FocalLength)))
    lens_width = F(k.LensHeight) * aspect
    ro = (np.full((H, W), pos[0]), np.full((H, W), pos[1]), np.full((H, W), pos[2]))
    ro = add(ro, div(mul(mul(vec(k.CameraRight), u * F(2) - F(1)), lens_width), F(2)))
    ro = add(ro, div(mul(mul(vec(k.CameraUp), v * F(2) - F(1)), F(k.LensHeight)), F(2)))
    rd = normalize(sub(ro, focal))
    return ro, rd


@np.errstate(all="ignore")
def cylinder(ro, rd, pa, pb, ra):
    """iCylinder :34-77, its distance alone: -1 without a hit."""
    ba, oc = sub(pb, pa), sub(ro, pa)
    baba, bard, baoc = dot(ba, ba), dot(ba, rd), dot(ba, oc)
    k2 = baba - bard * bard
    k1 = baba * dot(oc, rd) - baoc * bard
    k0 = (baba * dot(oc, oc) - baoc * baoc) - (ra * ra) * baba
    h = k1 * k1 - k2 * k0
    miss = h < F(0)
    h = np.sqrt(h)
    t = (-k1 - h) / k2
    y = baoc + t * bard
    body = (y > F(0)) & (y < baba)
    t_cap = (np.where(y < F(0), F(0), baba) - baoc) / bard
    cap = np.abs(k1 + k2 * t_cap) < h
    return np.where(miss, F(-1), np.where(body, t, np.where(cap, t_cap, F(-1)))).astype(np.float32)


@np.errstate(all="ignore")
def cone(ro, rd, pa, pb, ra, rb):
    """iCappedCone :92-131, its distance alone."""
    ba, oa, ob = sub(pb, pa), sub(ro, pa), sub(ro, pb)
    m0, m1, m2, m3 = dot(ba, ba), dot(oa, ba), dot(ob, ba), dot(rd, ba)
    first = m1 < F(0)
    v = sub(mul(oa, m3), mul(rd, m1))
    cap_a = first & (dot(v, v) < ((ra * ra) * m3) * m3)
    t_a = -m1 / m3
    v = sub(mul(ob, m3), mul(rd, m2))
    cap_b = ~first & (m2 > F(0)) & (dot(v, v) < ((rb * rb) * m3) * m3)
    t_b = -m2 / m3
    m4, m5, rr = dot(rd, oa), dot(oa, oa), ra - rb
    hy = m0 + rr * rr
    k2 = m0 * m0 - (m3 * m3) * hy
    k1 = ((m0 * m0) * m4 - (m1 * m3) * hy) + (m0 * ra) * ((rr * m3) * F(1))
    k0 = ((m0 * m0) * m5 - (m1 * m1) * hy) + (m0 * ra) * ((rr * m1) * F(2) - m0 * ra)
    h = k1 * k1 - k2 * k0
    miss = h < F(0)
    t = (-k1 - np.sqrt(h)) / k2
    y = m1 + t * m3
    body = (y > F(0)) & (y < m0)
    return np.where(cap_a, t_a, np.where(cap_b, t_b, np.where(miss, F(-1), np.where(body, t, F(-1))))).astype(np.float32)


def ray_words(rays):
    """(n, 8) float32: Origin, Direction, HitT, BounceCount of a structured array or of anything of that shape."""
    r = np.ascontiguousarray(rays)
    return r.view(np.float32).reshape(-1, 8) if r.dtype.names else np.asarray(r, np.float32).reshape(-1, 8)


def overlay(k, rays, scene, world_pos=None):
    """The picture vis_overlay writes: scene (H, W, 4) float32, world_pos (H, W, 4) or None (no occluder)."""
    scene = np.asarray(scene, np.float32)
    rays = ray_words(rays)
    with np.errstate(all="ignore"):
        ro, rd = camera_rays(k)
        # :151-156
        occluder = np.full(scene.shape[:2], F(-1))
        if world_pos is not None:
            wp = (np.asarray(world_pos, np.float32)[..., 0], np.asarray(world_pos, np.float32)[..., 1], np.asarray(world_pos, np.float32)[..., 2])
            there = (np.abs(wp[0]) > F(0.0001)) | (np.abs(wp[1]) > F(0.0001)) | (np.abs(wp[2]) > F(0.0001))
            d = sub(wp, ro)
            occluder = np.where(there, np.sqrt(dot(d, d)), F(-1)).astype(np.float32)
        # :158-223
        vis = [np.zeros(scene.shape[:2], np.float32) for _ in range(3)]
        alpha = np.zeros(scene.shape[:2], np.float32)
        closest = np.full(scene.shape[:2], FAR)
        radius, depth = F(k.CylinderRadius), F(k.RayDepth)
        have = min(len(rays), MAX_RAYS)
        count = 0 if int(k.RayCount) < 0 else min(int(k.RayCount), have)
        for r in rays[:count]:
            bounce, hit_t = r[7], r[6]
            color = (F(0), F(0), F(1)) if bounce < F(0) else ((F(0), F(1), F(0)) if bounce <= F(1.1) else (F(1), F(1), F(0)))
            start, direction = vec(r[0:3]), vec(r[3:6])
            length = hit_t if hit_t > F(0) else FAR
            bounce = np.abs(bounce)
            if bounce > depth:
                continue
            length = length * np.fmin(F(1), depth - bounce)
            end = add(start, mul(direction, length))
            t = cylinder(ro, rd, start, end, radius)
            take = (t > F(0)) & (t < closest) & ((occluder < F(0)) | (t < occluder))
            closest = np.where(take, t, closest)
            # nCylinder :80-88
            pa, ba = sub(add(ro, mul(rd, t)), start), sub(end, start)
            baba, paba = dot(ba, ba), dot(pa, ba)
            n = div(sub(pa, div(mul(ba, paba), baba)), radius)
            s = np.abs(dot(n, rd))
            for c in range(3):
                vis[c] = np.where(take, F(0.2) + s * (color[c] - F(0.2)), vis[c]).astype(np.float32)
            alpha = np.where(take, F(0.75), alpha)
            if hit_t > F(0):
                t = cone(ro, rd, add(start, mul(direction, length * F(0.8))), end, radius * F(10), radius)
                take = (t > F(0)) & (t < closest) & ((occluder < F(0)) | (t < occluder))
                closest = np.where(take, t, closest)
                for c in range(3):
                    vis[c] = np.where(take, color[c], vis[c]).astype(np.float32)
                alpha = np.where(take, F(0.75), alpha)
        # :225
        out = scene.copy()
        for c in range(3):
            out[..., c] = scene[..., c] + alpha * (vis[c] - scene[..., c])
    return out


def to_rgba8(image):
    """The output stage's R8G8B8A8_UNORM store (post_kernels.hip): clamp with the non-NaN operand winning, scale, + 0.5, truncate; alpha 255."""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(image, np.float32)[..., :3], F(0)), F(1))
        out = np.empty(image.shape[:2] + (4,), np.uint8)
        out[..., :3] = (c * F(255) + F(0.5)).astype(np.uint32).astype(np.uint8)
    out[..., 3] = 255
    return out
