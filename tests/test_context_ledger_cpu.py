"""CPU only: the context's GPU resources followed through a ledger (tests/context_ledger.cpp).  The real host code of the context,
the scene upload, the trace scheduling, the frame sequencing, the halo and the read-back is linked against stubs of every HIP call
and every kernel launcher; the stubs record each live allocation, event and stream and abort on a release of one that is not live.
After a whole lifecycle, and after the same lifecycle with each allocation / event / stream creation failing in turn, the ledger
is empty, the failing entry point returned an error, a failed vxrt_create left no context, and has_scene implies the scene's arrays."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIP_SOURCES = ["api_context.hip", "api_halo.hip", "api_extract.hip", "api_trace.hip", "api_scene.hip", "api_frame.hip"]
HOST_SOURCES = ["scene_host.cpp", "vox_scene.cpp", "api_host.cpp", "scene_procedural.cpp"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")
def test_context_ledger_balances_with_and_without_failures(tmp_path):
    csrc = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")
    exe = str(tmp_path / "context_ledger")
    # host code only (no kernel is compiled or launched); the executable's own HIP entry points take precedence over the runtime's
    build = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-I" + csrc,
                            "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "context_ledger.cpp")] +
                           [os.path.join(csrc, s) for s in HIP_SOURCES + HOST_SOURCES] + ["-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "FINDING" not in run.stdout and run.stdout.startswith("ok 9 lifecycles, "), run.stdout[-3000:]
    assert int(run.stdout.split()[3]) >= 9 * 20      # every configuration makes more than 20 fallible calls: each was failed once
