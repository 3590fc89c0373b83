"""-m gpu: what the query entry points share (csrc/host/query_call.h): the refusal of a caller's device pointer, per entry
point and per array in the order the entry point checks them, and the host paths' staging, which is gone when the call returns.  One triangle from
caller arrays and 8 rays or points: the seam is the same for every size."""
import numpy as np
import pytest

import mesh_cases as mc

pytestmark = pytest.mark.gpu
INVALID = -1
N = 8


@pytest.fixture(scope="module")
def one_triangle_tb(built):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    p, i = mc.one_triangle()
    tb.LoadMeshes([api.Mesh(p, i)], mc.MATERIALS())
    yield tb
    tb.close()


def _end_of_segment(t):
    """The first address behind the allocation torch cut the tensor from: what tb_* finds with hipMemGetAddressRange.  This takes a segment of
    torch's allocator to be one hipMalloc, which holds for its default configuration and not for expandable segments: there the runtime's range
    may end elsewhere, a pointer before this end may be accepted, and the test below then fails on its message, having touched nothing outside
    memory the runtime maps."""
    import torch
    at = t.data_ptr()
    for seg in torch.cuda.memory_snapshot():
        if seg["address"] <= at < seg["address"] + seg["total_size"]:
            return seg["address"] + seg["total_size"]
    raise AssertionError("torch's allocator does not know the tensor's segment")


def test_every_device_array_is_refused_by_its_name_in_the_entry_points_order(one_triangle_tb):
    """Per entry point its arrays in the order it checks them: the earlier ones valid, this one and every later one a few bytes before the end of
    their allocation, so that what the call would read or write runs past it.  Several arrays are wrong at once and the refusal names one: the
    first the entry point checks.  An entry point that checked a later array before this one would name the later one."""
    import torch
    from tracerboy_amd import _ctypes_abi as abi, api
    C = api.C
    tb = one_triangle_tb
    L, ctx = tb._L, tb._ctx
    room = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")   # valid for every array below, read or written: no call gets as far as a kernel
    ok, end = room.data_ptr(), _end_of_segment(room)
    torch.cuda.synchronize()
    g1 = api.ProbeGrid((0, 0, 0), (1, 1, 1), (1, 1, 1)).c_struct()    # one probe: 128 B
    g2 = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2)).c_struct()    # 8 cells: 32 B
    rad = abi.TbRadianceCall(0, 1, 0.0, api.RADIANCE_RAY | api.RADIANCE_DEVICE)
    bake = abi.tb_bake_call(2, 2, 0, 1, 0, api.BAKE_DEVICE)           # 2 x 2 texels: 64 B; the scene's 3 vertices: 24 B of uv
    probes = abi.tb_probe_call(N, 0, 2, 0, 1, api.PROBES_DEVICE)
    advance = C.c_float(0.0)
    ND, WD = api.NEAREST_DEVICE, api.WINDING_DEVICE
    # entry point, its arrays in its order, the call; `back`: how far before the end the failing pointer stands where 16 B is too far or too near
    table = [
        ("tb_trace_rays", ("rays", "out"), lambda rays, out: L.tb_trace_rays(ctx, api.RAYS_CLOSEST | api.RAYS_DEVICE, N, rays, out), {}),
        ("tb_trace_rays", ("rays", "out"), lambda rays, out: L.tb_trace_rays(ctx, api.RAYS_OCCLUDED | api.RAYS_DEVICE, N, rays, out), {"out": 4}),
        ("tb_nearest_points", ("points", "out"), lambda points, out: L.tb_nearest_points(ctx, ND, N, points, out), {}),
        ("tb_bake_distance_field", ("out",), lambda out: L.tb_bake_distance_field(ctx, ND, C.byref(g2), np.inf, out), {}),
        ("tb_winding_numbers", ("points", "out"), lambda points, out: L.tb_winding_numbers(ctx, WD, N, points, 3.0, out), {}),
        ("tb_bake_winding_field", ("out",), lambda out: L.tb_bake_winding_field(ctx, WD, C.byref(g2), 3.0, out), {}),
        ("tb_nearest_points_winding", ("points", "out"), lambda points, out: L.tb_nearest_points_winding(ctx, ND, N, points, 3.0, out), {}),
        ("tb_bake_distance_field_winding", ("out",), lambda out: L.tb_bake_distance_field_winding(ctx, ND, C.byref(g2), np.inf, 3.0, out), {}),
        ("tb_trace_radiance", ("rays", "out"), lambda rays, out: L.tb_trace_radiance(ctx, None, 0.0, C.byref(rad), N, rays, out), {}),
        ("tb_make_camera_rays", ("out",), lambda out: L.tb_make_camera_rays(ctx, None, 0.0, 4, 2, 0, 0, 4, 2, 0, api.RADIANCE_DEVICE, out, C.byref(advance)), {}),
        ("tb_bake_lightmap", ("uv", "rgba_out"), lambda uv, rgba_out: L.tb_bake_lightmap(ctx, None, 0.0, C.byref(bake), uv, rgba_out), {"uv": 8}),
        ("tb_bake_probes", ("positions", "probes_out"), lambda positions, probes_out: L.tb_bake_probes(ctx, None, 0.0, C.byref(probes), positions, probes_out), {}),
        ("tb_sample_probes", ("probes", "points", "normals", "rgba_out"), lambda probes, points, normals, rgba_out:
            L.tb_sample_probes(ctx, api.PROBES_DEVICE, C.byref(g1), 2, 0.25, probes, N, points, normals, rgba_out), {}),
    ]
    before = tb.GetOption("debug_live_device_bytes")
    for entry, names, call, back in table:
        for first_bad, name in enumerate(names):
            pointers = {k: ok if at < first_bad else end - back.get(k, 16) for at, k in enumerate(names)}
            rc = call(**pointers)
            said = (L.tb_last_error(ctx) or b"").decode()
            assert rc == INVALID and said == "%s: %s: the array runs past its allocation" % (entry, name), (entry, name, rc, said)
    assert tb.GetOption("debug_live_device_bytes") == before, "a refused call kept device memory"


def test_host_paths_keep_nothing(one_triangle_tb):
    """Once a first call of each has made what belongs to the context or the scene (the any-hit and radiance work counters, the overflow stacks, the
    winding moments), a second call of a host path leaves the library's count of live device bytes where it found it."""
    from tracerboy_amd import api
    tb = one_triangle_tb
    rng = np.random.default_rng(11)
    o = rng.uniform(-1, 1, (N, 3)).astype(np.float32) + np.float32([0, 1, 3])
    d = np.tile(np.float32([0, 0, -1]), (N, 1))
    rays, rad_rays, points = api.make_query_rays(o, d), api.make_radiance_rays(o, d), api.make_query_points(o)
    grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    probe_records = np.zeros(grid.n, api.PROBE_DTYPE)
    calls = {
        "TraceRays closest": lambda: tb.TraceRays(rays, api.RAYS_CLOSEST),
        "TraceRays occluded": lambda: tb.TraceRays(rays, api.RAYS_OCCLUDED),
        "NearestPoints": lambda: tb.NearestPoints(points),
        "BakeDistanceField": lambda: tb.BakeDistanceField(grid),
        "WindingNumbers": lambda: tb.WindingNumbers(points),
        "TraceRadiance": lambda: tb.TraceRadiance(rad_rays, samples=2),
        "MakeCameraRays": lambda: tb.MakeCameraRays(4, 2, 0),
        "SampleProbes": lambda: tb.SampleProbes(grid, probe_records, o, d, resolution=2),
    }
    first = {what: call() for what, call in calls.items()}
    for what, call in calls.items():
        before = tb.GetOption("debug_live_device_bytes")
        again = call()
        assert tb.GetOption("debug_live_device_bytes") == before, "%s: %d B outlive the call" % (what, tb.GetOption("debug_live_device_bytes") - before)
        a, b = (first[what], again) if what != "MakeCameraRays" else (first[what][0], again[0])
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: the second call answers in another form" % what
    assert first["TraceRays closest"].dtype == api.QUERY_HIT_DTYPE and first["TraceRays occluded"].dtype == np.uint8
    assert first["NearestPoints"].dtype == api.NEAREST_DTYPE and first["MakeCameraRays"][0].dtype == api.RADIANCE_RAY_DTYPE
