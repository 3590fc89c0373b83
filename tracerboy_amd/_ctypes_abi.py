"""ctypes mirrors of include/tb_abi.h and include/tracerboy_hip.h (POD layouts only, no logic)."""
import ctypes as C

# tb_read_guide selectors (include/tracerboy_hip.h, the guide pass)
TB_GUIDE_ALBEDO, TB_GUIDE_NORMAL, TB_GUIDE_POSITION = 0, 1, 2


class TbFloat2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class TbFloat3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class TbFloat4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class TbPerFrameConstants(C.Structure):
    _fields_ = [
        ("CameraPosition", TbFloat3), ("Time", C.c_float),
        ("CameraLookAt", TbFloat3), ("InvalidateHistory", C.c_uint32),
        ("CameraUp", TbFloat3), ("OutputMode", C.c_uint32),
        ("CameraRight", TbFloat3), ("DOFFocusDistance", C.c_float),
        ("DOFApertureWidth", C.c_float), ("EnableNormalMaps", C.c_uint32), ("FocalDistance", C.c_float), ("FireflyClampValue", C.c_float),
        ("GlobalFrameCount", C.c_uint32), ("MinConvergence", C.c_float), ("LightCount", C.c_uint32), ("UseBlueNoise", C.c_uint32),
        ("IsRealTime", C.c_uint32), ("EnableNextEventEstimation", C.c_uint32), ("EnableSamplingImportanceResampling", C.c_uint32), ("FilterWidth", C.c_float),
        ("FilterType", C.c_uint32), ("SelectedPixelX", C.c_uint32), ("SelectedPixelY", C.c_uint32), ("MaxZ", C.c_float),
        ("FixedPixelOffset", TbFloat2), ("DebugValue", C.c_float), ("DebugValue2", C.c_float),
        ("MaxBounces", C.c_uint32),
    ]


class TbConfigConstants(C.Structure):
    _fields_ = [("CameraLensHeight", C.c_float), ("FlipTextureUVs", C.c_uint32), ("Padding", TbFloat2),
                ("EnvMapTransformVx", TbFloat4), ("EnvMapTransformVy", TbFloat4), ("EnvMapTransformVz", TbFloat4),
                ("EnvironmentMapColorScale", TbFloat3)]


class TbLight(C.Structure):
    _fields_ = [("LightType", C.c_uint32), ("LightColor", TbFloat3), ("SurfaceArea", C.c_float),
                ("P0", TbFloat3), ("P1", TbFloat3), ("P2", TbFloat3), ("N0", TbFloat3), ("N1", TbFloat3), ("N2", TbFloat3),
                ("Direction", TbFloat3)]


class TbMaterial(C.Structure):
    _fields_ = [("albedo", TbFloat3), ("albedoIndex", C.c_uint32),
                ("alphaIndex", C.c_uint32), ("normalMapIndex", C.c_uint32), ("emissiveIndex", C.c_uint32), ("specularMapIndex", C.c_uint32),
                ("IOR", C.c_float), ("absorption", TbFloat3),
                ("roughness", C.c_float), ("scattering", TbFloat3),
                ("emissive", TbFloat3), ("Flags", C.c_int32),
                ("SpecularCoef", C.c_float)]


class TbTextureData(C.Structure):
    _fields_ = [("TextureType", C.c_uint32), ("DescriptorHeapIndex", C.c_uint32), ("TextureFlags", C.c_uint32), ("Padding", C.c_uint32),
                ("CheckerColor1", TbFloat3), ("UScale", C.c_float), ("CheckerColor2", TbFloat3), ("VScale", C.c_float),
                ("TextureIndex1", C.c_uint32), ("ScaleColor1", TbFloat3), ("TextureIndex2", C.c_uint32), ("ScaleColor2", TbFloat3)]


class TbHitGroupRecord(C.Structure):
    _fields_ = [("ShaderIdentifier", C.c_uint32 * 8), ("MaterialIndex", C.c_uint32), ("VertexBufferIndex", C.c_uint32),
                ("VertexBufferOffset", C.c_uint32), ("IndexBufferIndex", C.c_uint32), ("IndexBufferOffset", C.c_uint32),
                ("GeometryIndex", C.c_uint32), ("Padding", C.c_uint32 * 4)]


class TbNodeB(C.Structure):
    _fields_ = [("cx", C.c_float * 2), ("cy", C.c_float * 2), ("cz", C.c_float * 2), ("hx", C.c_float * 2), ("hy", C.c_float * 2), ("hz", C.c_float * 2),
                ("left", C.c_uint32), ("right", C.c_uint32), ("pad", C.c_uint32 * 2)]


class TbTriB(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("geometryIndex", C.c_uint32), ("v1", C.c_float * 3), ("primitiveIndex", C.c_uint32),
                ("v2", C.c_float * 3), ("geometryFlags", C.c_uint32)]


class TbImageDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texelOffset", C.c_uint64)]


class TbSceneView(C.Structure):
    _fields_ = [
        ("bvh", C.c_void_p), ("bvhBytes", C.c_uint32), ("numTriangles", C.c_uint32),
        ("hitGroups", C.POINTER(TbHitGroupRecord)), ("numHitGroups", C.c_uint32),
        ("indexBuffer", C.POINTER(C.c_uint32)), ("numIndices", C.c_uint32),
        ("vertexBuffer", C.POINTER(C.c_float)), ("numVertexFloats", C.c_uint32),
        ("materials", C.POINTER(TbMaterial)), ("numMaterials", C.c_uint32),
        ("textureData", C.POINTER(TbTextureData)), ("numTextureData", C.c_uint32),
        ("lights", C.POINTER(TbLight)), ("numLights", C.c_uint32),
        ("images", C.POINTER(TbImageDesc)), ("numImages", C.c_uint32),
        ("texelPool", C.POINTER(TbFloat4)),
        ("envMap", C.POINTER(TbFloat4)), ("envWidth", C.c_uint32), ("envHeight", C.c_uint32),
        ("blueNoise0", C.POINTER(TbFloat4)), ("blueNoise1", C.POINTER(TbFloat4)),
        ("config", TbConfigConstants),
        ("tlas", C.c_void_p), ("tlasBytes", C.c_uint32), ("numInstances", C.c_uint32), ("numBlas", C.c_uint32),
        ("blasOffsets", C.POINTER(C.c_uint32)),
    ]


class TbBvhMetadata(C.Structure):
    _fields_ = [("WorldToObject", C.c_float * 12), ("InstanceIDAndMask", C.c_uint32), ("InstanceContributionToHitGroupIndexAndFlags", C.c_uint32),
                ("BlasIndex", C.c_uint32), ("BlasPad", C.c_uint32), ("ObjectToWorld", C.c_float * 12), ("InstanceIndex", C.c_uint32)]


class TbRayStats(C.Structure):
    _fields_ = [("boxesTested", C.c_uint64), ("trianglesTested", C.c_uint64), ("hitsShaded", C.c_uint64), ("materialFetches", C.c_uint64),
                ("lightSamples", C.c_uint64), ("samples", C.c_uint64), ("rays", C.c_uint64)]


class tb_camera(C.Structure):
    _fields_ = [("Position", C.c_float * 3), ("LookAt", C.c_float * 3), ("Right", C.c_float * 3), ("Up", C.c_float * 3),
                ("LensHeight", C.c_float), ("FocalDistance", C.c_float)]


class tb_output_settings(C.Structure):
    _fields_ = [("OutputType", C.c_uint32), ("EnableNormalMaps", C.c_uint32), ("RenderModeRealTime", C.c_uint32),
                ("DebugValue", C.c_float), ("DebugValue2", C.c_float),
                ("DOFFocalDistance", C.c_float), ("ApertureWidth", C.c_float), ("FilterType", C.c_uint32), ("FilterWidth", C.c_float),
                ("FireflyClampValue", C.c_float), ("MaxZ", C.c_float), ("ConvergencePercentage", C.c_float),
                ("EnableNextEventEstimation", C.c_uint32), ("EnableSamplingImportanceResampling", C.c_uint32), ("EnableBlueNoise", C.c_uint32),
                ("MaxBounces", C.c_int32), ("SampleTarget", C.c_int32)]


class tb_post_settings(C.Structure):
    _fields_ = [("ExposureMultiplier", C.c_float), ("EnableGammaCorrection", C.c_uint32), ("EnableAutoExposure", C.c_uint32),
                ("TonemapType", C.c_uint32), ("VarianceMultiplier", C.c_float)]


class TbPostConstants(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("FramesRendered", C.c_uint32), ("ExposureMultiplier", C.c_float),
                ("TonemapType", C.c_uint32), ("UseGammaCorrection", C.c_uint32), ("UseAutoExposure", C.c_uint32), ("OutputType", C.c_uint32),
                ("VarianceMultiplier", C.c_float)]


class tb_denoiser_settings(C.Structure):
    _fields_ = [("Enabled", C.c_uint32), ("IntersectPositionWeightingMultiplier", C.c_float), ("NormalWeightingExponential", C.c_float),
                ("LuminanceWeightingMultiplier", C.c_float), ("WaveletIterations", C.c_uint32)]


class TbTemporalConstants(C.Structure):
    _fields_ = [("ResolutionX", C.c_uint32), ("ResolutionY", C.c_uint32), ("CameraFocalDistance", C.c_float), ("IgnoreHistory", C.c_uint32),
                ("CameraPosition", C.c_float * 3), ("CameraLensHeight", C.c_float), ("CameraLookAt", C.c_float * 3), ("HistoryWeight", C.c_float),
                ("CameraUp", C.c_float * 3), ("OutputMomentInformation", C.c_uint32), ("CameraRight", C.c_float * 3), ("padding3", C.c_uint32),
                ("PrevFrameCameraPosition", C.c_float * 3), ("padding4", C.c_uint32), ("PrevFrameCameraUp", C.c_float * 3), ("padding5", C.c_uint32),
                ("PrevFrameCameraRight", C.c_float * 3), ("padding6", C.c_uint32), ("PrevFrameCameraLookAt", C.c_float * 3), ("padding7", C.c_uint32)]


class TbDenoiserConstants(C.Structure):
    _fields_ = [("ResolutionX", C.c_uint32), ("ResolutionY", C.c_uint32), ("OffsetMultiplier", C.c_uint32), ("NormalWeightingExponential", C.c_float),
                ("IntersectionPositionWeightingMultiplier", C.c_float), ("LumaWeightingMultiplier", C.c_float), ("GlobalFrameCount", C.c_uint32)]


class TbFsrConstants(C.Structure):
    """FsrEasuCon's const0..const3 and FsrRcasCon's const0 (tb_abi.h)."""
    _fields_ = [("easu", C.c_uint32 * 16), ("rcas", C.c_uint32 * 4)]


TB_FSR_SURFACE_UNORM8 = 0
TB_FSR_SURFACE_F32 = 1


# the path inspector (include/tb_abi.h)
TB_MAX_VISUALIZER_RAYS = 1024
TB_PATH_JITTERED, TB_PATH_REJECTED, TB_PATH_TRUNCATED = 1, 2, 4


class TbVisualizerRay(C.Structure):
    """A record of the reference's ray buffer (VisualizationRaysCommon.h)."""
    _fields_ = [("Origin", C.c_float * 3), ("Direction", C.c_float * 3), ("HitT", C.c_float), ("BounceCount", C.c_float)]


class TbPathFrame(C.Structure):
    """One frame of a recorded pixel (tb_record_paths)."""
    _fields_ = [("sum", C.c_float * 4), ("frame", C.c_uint32), ("first_ray", C.c_uint32), ("num_rays", C.c_uint32), ("flags", C.c_uint32)]


class TbVisualizeConstants(C.Structure):
    """VisualizationRaysConstants (VisualizeRaysSharedShaderStructs.h)."""
    _fields_ = [("ResolutionX", C.c_uint32), ("ResolutionY", C.c_uint32), ("CylinderRadius", C.c_float), ("FocalLength", C.c_float),
                ("CameraPosition", C.c_float * 3), ("LensHeight", C.c_float), ("CameraLookAt", C.c_float * 3), ("RayDepth", C.c_float),
                ("CameraRight", C.c_float * 3), ("Padding2", C.c_float), ("CameraUp", C.c_float * 3), ("RayCount", C.c_int32)]


class tb_visualize_settings(C.Structure):
    """include/tracerboy_hip.h tb_visualize_settings: m_VisualizeRayWidth / m_VisualizeRayDepth / m_VisualizeRayCount (TracerBoy.h:303-306)."""
    _fields_ = [("RayWidth", C.c_float), ("RayDepth", C.c_float), ("RayCount", C.c_int32)]


class TbQueryRay(C.Structure):
    """A ray of tb_trace_rays (tb_abi.h): a candidate counts iff MIN_T < t < min(TMax, MAX_T); Flags bit 0 = not traced."""
    _fields_ = [("Origin", C.c_float * 3), ("TMax", C.c_float), ("Direction", C.c_float * 3), ("Flags", C.c_uint32)]


class TbQueryHit(C.Structure):
    """A hit record of tb_trace_rays (tb_abi.h): tb_trace_closest's fields; T = -1 for a miss."""
    _fields_ = [("T", C.c_float), ("U", C.c_float), ("V", C.c_float), ("Prim", C.c_uint32), ("Geom", C.c_uint32), ("Material", C.c_int32),
                ("UV", C.c_float * 2), ("Normal", C.c_float * 3), ("Pad", C.c_uint32)]


class TbRadianceRay(C.Structure):
    """A ray of tb_trace_radiance (tb_abi.h): where a path starts, its unit direction (hemisphere mode: the unit normal), the seed's two coordinates."""
    _fields_ = [("Origin", C.c_float * 3), ("SeedX", C.c_float), ("Direction", C.c_float * 3), ("SeedY", C.c_float)]


class TbRadianceCall(C.Structure):
    """A call of tb_trace_radiance (tb_abi.h): the samples [first_sample, first_sample + num_samples), the seed's advance, TB_RADIANCE_* mode | flags."""
    _fields_ = [("first_sample", C.c_uint32), ("num_samples", C.c_uint32), ("seed_advance", C.c_float), ("mode_and_flags", C.c_uint32)]


class TbBakeTexel(C.Structure):
    """What the lightmap rasteriser found for a texel (tb_abi.h): the triangle (0xffffffff: none), the class, the weights of its vertices 0 and 1."""
    _fields_ = [("triangle", C.c_uint32), ("cls", C.c_uint32), ("w0", C.c_float), ("w1", C.c_float)]


class tb_bake_call(C.Structure):
    """A call of tb_bake_lightmap (tracerboy_hip.h): the atlas, the samples [first_sample, first_sample + num_samples), the fill passes, TB_BAKE_* flags."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("first_sample", C.c_uint32), ("num_samples", C.c_uint32),
                ("dilate_passes", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(TbBakeTexel) == 16 and C.sizeof(tb_bake_call) == 24


class TbProbe(C.Structure):
    """One light probe (tb_abi.h): 27 SH coefficients (j * 3 + channel), then the weight sum and the hit statistics."""
    _fields_ = [("SH", C.c_float * 27), ("Weight", C.c_float), ("Hits", C.c_float), ("Backfaces", C.c_float), ("MinDistance", C.c_float),
                ("MeanDistance", C.c_float)]


class tb_probe_grid(C.Structure):
    """A grid of probes (tb_abi.h): probe (i, j, k) has the number (k * count[1] + j) * count[0] + i and sits at origin + (i, j, k) * spacing."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("count", C.c_uint32 * 3)]


class tb_probe_call(C.Structure):
    """A call of tb_bake_probes (tracerboy_hip.h): n probes numbered from first_probe_number, the map's resolution, the samples
    [first_sample, first_sample + num_samples), TB_PROBES_* flags."""
    _fields_ = [("n", C.c_uint32), ("first_probe_number", C.c_uint32), ("resolution", C.c_uint32), ("first_sample", C.c_uint32),
                ("num_samples", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(TbProbe) == 128 and C.sizeof(tb_probe_grid) == 36 and C.sizeof(tb_probe_call) == 24


class TbQueryPoint(C.Structure):
    """A point of tb_nearest_points (tb_abi.h): a triangle counts iff the Distance of its record is <= MaxDistance."""
    _fields_ = [("Position", C.c_float * 3), ("MaxDistance", C.c_float)]


class TbNearest(C.Structure):
    """A record of tb_nearest_points (tb_abi.h): the nearest point, its distance, the weights of the triangle's vertices 1 and 2; a miss is
    Point = 0, Distance = +inf, U = V = 0, Prim = Geom = 0xffffffff."""
    _fields_ = [("Point", C.c_float * 3), ("Distance", C.c_float), ("U", C.c_float), ("V", C.c_float), ("Prim", C.c_uint32), ("Geom", C.c_uint32)]


assert C.sizeof(TbQueryPoint) == 16 and C.sizeof(TbNearest) == 32


class tb_nn_info(C.Structure):
    """include/tracerboy_hip.h tb_nn_info: the channel counts of a weights file's 16 layers (tb_nn_weights_info)."""
    _fields_ = [("in_channels", C.c_uint32), ("out_channels", C.c_uint32 * 16), ("in_channels_of", C.c_uint32 * 16), ("weight_bytes", C.c_uint64)]


class tb_conv3x3_desc(C.Structure):
    """include/tracerboy_hip.h tb_conv3x3_desc: one layer of the neural denoiser at the layer seam (tb_run_conv3x3)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "c_a", "c_b", "c_out", "upsample_a", "pool", "relu")]


class tb_sr_info(C.Structure):
    """include/tracerboy_hip.h tb_sr_info: the channel counts and filter sizes of a super-resolution weights file's 7 layers (tb_sr_weights_info)."""
    _fields_ = [("in_channels", C.c_uint32 * 7), ("out_channels", C.c_uint32 * 7), ("kernel", C.c_uint32 * 7), ("weight_bytes", C.c_uint64)]


class tb_conv_desc(C.Structure):
    """include/tracerboy_hip.h tb_conv_desc: one 3 x 3 or 5 x 5 layer at the layer seam (tb_run_conv)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "c_a", "c_b", "c_out", "kernel", "upsample_a", "relu", "form")]


TB_UPDATE_DEVICE, TB_GEOMETRY_REBUILD = 0x100, 1  # include/tracerboy_hip.h: tb_update_positions / tb_update_normals flags; tb_commit_geometry flags
TB_MESH_NORMALS_FLAT, TB_MESH_NORMALS_SMOOTH, TB_MESH_DEVICE = 0, 1, 0x100  # include/tb_abi.h: tb_mesh_desc.normals_mode; tb_scene_desc.flags


class tb_mesh_desc(C.Structure):
    """include/tb_abi.h tb_mesh_desc: one mesh of a scene from arrays (tb_load_meshes)."""
    _fields_ = [("positions", C.c_void_p), ("n_vertices", C.c_uint32), ("indices", C.c_void_p), ("n_triangles", C.c_uint32),
                ("normals_or_null", C.c_void_p), ("uvs_or_null", C.c_void_p), ("material", C.c_uint32), ("normals_mode", C.c_uint32)]


class tb_scene_desc(C.Structure):
    """include/tb_abi.h tb_scene_desc: the meshes, materials, camera, environment and film of a scene from arrays."""
    _fields_ = [("meshes", C.POINTER(tb_mesh_desc)), ("n_meshes", C.c_uint32), ("materials", C.POINTER(TbMaterial)), ("n_materials", C.c_uint32),
                ("camera_or_null", C.POINTER(tb_camera)), ("env_rgba_or_null", C.c_void_p), ("env_width", C.c_uint32), ("env_height", C.c_uint32),
                ("env_scale", C.c_float * 3), ("film_width", C.c_uint32), ("film_height", C.c_uint32), ("flags", C.c_uint32)]
TB_COMPARE_SSIM, TB_COMPARE_SUMS = 1, 2          # tb_compare_settings.flags
TB_COMPARE_MEAN, TB_COMPARE_DENOISED = 0, 1      # tb_compare's surface


class tb_compare_settings(C.Structure):
    """include/tracerboy_hip.h tb_compare_settings: what the image-quality metrics are told."""
    _fields_ = [("peak", C.c_float), ("rel_epsilon", C.c_float), ("flags", C.c_uint32)]


class tb_compare_result(C.Structure):
    """include/tracerboy_hip.h tb_compare_result: the metrics of one comparison."""
    _fields_ = [(n, C.c_uint64) for n in ("pixels", "excluded", "unsampled", "ssim_windows", "ssim_windows_skipped")] + \
               [(n, C.c_double) for n in ("mse", "mae", "rel_mse", "max_abs", "psnr", "ssim")] + [("gpu_us", C.c_float)]


class tb_readback_stats(C.Structure):
    _fields_ = [("ActiveWaves", C.c_uint32), ("ActivePixels", C.c_uint32), ("SelectedPixelDistance", C.c_float), ("SelectedMaterialID", C.c_int32),
                ("rays", TbRayStats)]


class tb_scene_info(C.Structure):
    _fields_ = [("numTriangles", C.c_uint32), ("numVertices", C.c_uint32), ("numMaterials", C.c_uint32), ("numLights", C.c_uint32),
                ("numGeometries", C.c_uint32), ("numTextures", C.c_uint32), ("bvhBytesA", C.c_uint32), ("bvhNodesB", C.c_uint32),
                ("bvhMaxDepth", C.c_uint32), ("filmWidth", C.c_uint32), ("filmHeight", C.c_uint32),
                ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3)]


class tb_lds_image_info(C.Structure):
    """include/tracerboy_hip.h tb_lds_image_info: the sections of the walk's LDS image (tb_host_scene_lds_image)."""
    _fields_ = [(n, C.c_uint32) for n in ("bytes", "off_nodes", "off_tris", "num_nodes", "num_tris", "node_stride", "tri_copies", "root_ref", "stack_depth")]


class tb_wave_trips(C.Structure):
    """include/tracerboy_hip.h tb_wave_trips: what a 64-lane wave pays for a set of walks (csrc/host/wave_cost.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("inner_trips", "leaf_trips", "idle_passes", "inner_active", "leaf_active")] + [("cost", C.c_double)]


class tb_wave_stage_info(C.Structure):
    """include/tracerboy_hip.h tb_wave_stage_info: what builder 1's wave stage did when a host scene was built."""
    _fields_ = [(n, C.c_uint32) for n in ("ran", "rays", "seed", "park_min", "depth_limit", "moves", "evaluations", "inner_insts", "leaf_insts",
                                          "reserved")] + [("before", tb_wave_trips), ("after", tb_wave_trips), ("milliseconds", C.c_double)] + \
               [(n, C.c_uint64) for n in ("places_priced", "abandoned", "rays_checked", "rays_rewalked", "places_screened")] + \
               [(n, C.c_uint32) for n in ("threads", "passes", "places", "validation_rejects", "cuts_skipped", "screen_waves", "screen_keep", "reserved2")] + \
               [("validation_before", C.c_double), ("validation_after", C.c_double)]


class tb_state_info(C.Structure):
    """include/tracerboy_hip.h tb_state_info: the header of a render-state file."""
    _fields_ = [("version", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("first_frame", C.c_uint32), ("next_frame", C.c_uint32),
                ("time_seed", C.c_float), ("settings", tb_output_settings), ("camera", tb_camera),
                ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("alpha_test", C.c_uint32), ("adaptive", C.c_uint32), ("adaptive_test", C.c_uint32),
                ("adaptive_min_frames", C.c_int64), ("scene_digest", C.c_uint64), ("output_digest", C.c_uint64), ("jittered_digest", C.c_uint64)]


class tb_plan_input(C.Structure):
    """include/tracerboy_hip.h tb_plan_input: what the launch policy is told (scene statistics, the call, the options)."""
    _fields_ = [("variant_features", C.c_uint32), ("variant_waves_hi", C.c_uint32), ("variant_prepass_in_base", C.c_uint32),
                ("variant_has_wavefront", C.c_uint32), ("variant_has_pooled", C.c_uint32), ("variant_has_split", C.c_uint32), ("variant_stash_entries", C.c_uint32),
                ("scene_in_lds", C.c_uint32), ("lds_blob_bytes", C.c_uint32), ("stack_depth", C.c_uint32), ("two_level", C.c_uint32), ("has_lights", C.c_uint32),
                ("has_compact_nodes", C.c_uint32), ("interior_walk_triangle_share", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32), ("frames", C.c_uint32), ("max_bounces", C.c_int32), ("owned_regions", C.c_uint64),
                ("count_rays", C.c_uint32), ("aov", C.c_uint32), ("realtime", C.c_uint32), ("selected_pixel", C.c_uint32),
                ("pipeline", C.c_int64), ("frame_group", C.c_int64), ("high_occupancy", C.c_int64), ("stack_lds_cap", C.c_int64), ("stack_overflow_max", C.c_int64),
                ("node_layout", C.c_int64), ("primary_prepass", C.c_int64), ("overlap_launches", C.c_int64), ("pooled_samples", C.c_int64),
                ("split_trav", C.c_int64), ("split_shade", C.c_int64), ("split_stack_cap", C.c_int64), ("guided_groups", C.c_int64), ("sync_call", C.c_uint32), ("costly_first", C.c_uint32),
                ("adaptive", C.c_uint32)]


class tb_launch_plan(C.Structure):
    _fields_ = [("pipeline", C.c_int32), ("groups", C.c_uint32), ("high_occupancy_copy", C.c_uint32), ("full_variant", C.c_uint32),
                ("stack_lds_entries", C.c_uint32), ("stack_overflow_entries", C.c_uint32), ("compact_nodes", C.c_uint32), ("prepass", C.c_uint32),
                ("overlap_launches", C.c_uint32), ("batch_frames", C.c_uint32), ("frame_group", C.c_uint32),
                ("rule_pipeline", C.c_uint32), ("rule_copy", C.c_uint32), ("rule_prepass", C.c_uint32), ("guided_groups", C.c_uint32), ("costly_first", C.c_uint32)]


assert C.sizeof(tb_state_info) == 208
assert C.sizeof(TbPostConstants) == 36
assert C.sizeof(TbTemporalConstants) == 144
assert C.sizeof(TbDenoiserConstants) == 28
assert C.sizeof(TbFsrConstants) == 80
assert C.sizeof(TbVisualizerRay) == 32 and C.sizeof(TbVisualizeConstants) == 80 and C.sizeof(TbPathFrame) == 32
assert C.sizeof(tb_visualize_settings) == 12
assert C.sizeof(TbQueryRay) == 32 and C.sizeof(TbQueryHit) == 48
assert C.sizeof(TbRadianceRay) == 32 and C.sizeof(TbRadianceCall) == 16
assert C.sizeof(tb_compare_settings) == 12 and C.sizeof(tb_compare_result) == 96
assert C.sizeof(TbPerFrameConstants) == 148
assert C.sizeof(TbConfigConstants) == 76
assert C.sizeof(TbLight) == 104
assert C.sizeof(TbMaterial) == 84
assert C.sizeof(TbTextureData) == 80
assert C.sizeof(TbHitGroupRecord) == 72
assert C.sizeof(TbNodeB) == 64
assert C.sizeof(TbTriB) == 48
