"""The matte feature set's copy for scenes in LDS (pt_variant_matte6.hip): six waves per SIMD, frame-group kernels with the whole stack in LDS.

CPU: the code object of the shipped copy holds few enough VGPRs for the wave count the library reports (tb_variant_waves_lds).
GPU: cornell-box at the bench's size runs that copy with the whole stack in LDS, and a small frame through it is bit-equal to the base copy and
to the CPU oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, ROOT

LLVM = "/opt/rocm/llvm/bin"
OBJ = os.path.join(ROOT, "tracerboy_amd", "_build", "kernels_pt_variant_matte6.hip.o")


def _kernel_notes(obj, tmp_path):
    """[(kernel name, vgpr_count, group_segment_fixed_size)] of the gfx950 code object inside a hipcc object file"""
    fatbin, co = str(tmp_path / "fatbin.bin"), str(tmp_path / "matte6.co")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section=.hip_fatbin=" + fatbin, obj, str(tmp_path / "host.o")], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fatbin,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for block in notes.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
        out.append((f["name"], int(f["vgpr_count"]), int(f["group_segment_fixed_size"])))
    return out


def test_lds_copy_registers_admit_its_waves(built, tmp_path):
    from tracerboy_amd import api
    waves = api.VariantWavesLds("matte")
    assert waves == 6 and api.VariantWavesLds("env") == 0 and api.VariantWavesLds("nope") == -1
    kernels = _kernel_notes(OBJ, tmp_path)
    assert kernels and all("pt_persistent" in name for name, _, _ in kernels)
    for name, vgprs, static_lds in kernels:
        # 512 VGPRs per SIMD lane on gfx950, allocated in granules of 8: six waves need <= 80
        assert 512 // ((vgprs + 7) // 8 * 8) >= waves, (name, vgprs)
        assert static_lds <= 128, (name, static_lds)   # the plan's LDS arithmetic counts 128 B of static LDS (launch_plan.h)


@pytest.mark.gpu
def test_cornell_bench_size_runs_the_lds_copy_with_the_whole_stack(gpu_tb):
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings(); s.MaxBounces = 8
    gpu_tb.LoadScene(CORNELL)
    assert gpu_tb.GetOption("scene_in_lds_active") == 1
    for sync in (True, False):   # a call that waits (groups that shrink at the end) and the bench's asynchronous one
        gpu_tb.InvalidateHistory()
        gpu_tb.Render(1920, 1080, 64, s, 0.0, sync=sync)
        gpu_tb.Sync()
        assert gpu_tb.GetOption("last_variant") == 0 and gpu_tb.GetOption("last_pipeline") == 0
        assert gpu_tb.GetOption("last_plan_rule_copy") == 11                 # TB_PLAN_RULE_COPY_FITS
        assert gpu_tb.GetOption("last_plan_stack_overflow") == 0
        assert gpu_tb.GetOption("last_copy_waves") == api.VariantWavesLds("matte"), sync


@pytest.mark.gpu
def test_lds_copy_is_bit_equal_to_the_base_copy_and_the_oracle(gpu_tb, settings):
    import oracle_lib as ol
    W, H, F = 96, 80, 6
    gpu_tb.LoadScene(CORNELL)
    gpu_tb.InvalidateHistory(); gpu_tb.Render(W, H, F, settings, 0.0)
    assert gpu_tb.GetOption("last_copy_waves") == 6
    lds_copy, lds_jit = gpu_tb.ReadAccumulation(jittered=True)
    gpu_tb.SetOption("high_occupancy", 0)
    try:
        gpu_tb.InvalidateHistory(); gpu_tb.Render(W, H, F, settings, 0.0)
        assert gpu_tb.GetOption("last_copy_waves") == 0
        base, base_jit = gpu_tb.ReadAccumulation(jittered=True)
    finally:
        gpu_tb.SetOption("high_occupancy", 1)
    ref = ol.render(gpu_tb.HostSceneView(), gpu_tb.FrameConstants(W, H, 0, settings, 0.0), W, H, F, threads=8, jittered=True)
    assert np.array_equal(lds_copy.view(np.uint32), base.view(np.uint32))
    assert np.array_equal(lds_jit.view(np.uint32), base_jit.view(np.uint32))
    assert np.array_equal(lds_copy.view(np.uint32), ref["output"].view(np.uint32))
    assert np.array_equal(lds_jit.view(np.uint32), ref["jittered"].view(np.uint32))
