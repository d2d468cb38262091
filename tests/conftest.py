import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = "/root/reference"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # the parity tests of the scheduling variants name them by the VXRT_* variables the A/B scripts use; the library reads no
    # environment, the host layer translates them into vxrt_create_tuned options when asked to (host.enable_env_knobs)
    from gpu_voxel_raytracer_amd import host
    host.enable_env_knobs()


@pytest.fixture(scope="session")
def O():
    """The CPU oracle (test infrastructure).  Built on demand with g++."""
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="session")
def H():
    """The product's host layer (ctypes over libvxrt.so)."""
    from gpu_voxel_raytracer_amd import host
    host.lib()
    return host


@pytest.fixture(scope="session")
def noise(O):
    return O.noise_table()


@pytest.fixture(scope="session")
def scenes():
    from gpu_voxel_raytracer_amd import scenes as s
    return s


def require_variants(H, env=None, tracer=None, wide=None):
    """A case that needs a schedule or scene format the product library does not hold (tracers 2 / 3 / 5, the wide records: compiled
    only with -DVXRT_VARIANTS=1) runs in libvxrt_variants.so, loaded beside the product for the length of the test (round 5; until
    then these cases were skipped unless VXRT_LIB pointed at that build).  The autouse fixture below switches back."""
    env = env or {}
    needs = (str(env.get("VXRT_TRACE_VARIANT", "")) in ("2", "3", "5") or str(env.get("VXRT_WIDE", "")) == "1" or str(env.get("VXRT_FUSED_TAIL", "")) == "1" or str(env.get("VXRT_LONG_TILES", "0")) != "0" or
             str(tracer) in ("2", "3", "5") or str(wide) in ("1", "True", "wide"))
    if needs and not H.has_variants():
        H.use_library(H.variants_library())
        assert H.has_variants()


@pytest.fixture(autouse=True)
def _product_library_after_each_test():
    """Whatever library was in use before a test — the product, or the A/B build VXRT_LIB names — is in use again after it (ADVICE r5:
    with VXRT_LIB set, the session used to stay on libvxrt_variants.so after the first case that had asked for it)."""
    from gpu_voxel_raytracer_amd import host
    before = host._LIB
    yield
    if host._LIB is not before:
        host._LIB = before           # None: lib() resolves it again on next use


def have_reference():
    return os.path.isdir(os.path.join(REFERENCE, "vox"))


needs_reference = pytest.mark.skipif(not have_reference(), reason="/root/reference not mounted (GPU box)")

# the reference's scene files, byte for byte (xz-compressed data fixtures; octree_kat.json pins each one's sha256)
VOX_FIXTURES = os.path.join(GOLDEN, "vox")


def reference_vox_names():
    return sorted(f[:-len(".vox.xz")] for f in os.listdir(VOX_FIXTURES) if f.endswith(".vox.xz"))


def reference_vox(name):
    import lzma
    with lzma.open(os.path.join(VOX_FIXTURES, name + ".vox.xz")) as f:
        return f.read()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what=""):
    """Bitwise equality of float images, except that +0/-0 and NaN payloads are not distinguished."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    if not same.all():
        idx = np.argwhere(~same)
        first = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} of {a.size} values differ; first at {first}: {a[first]!r} vs {b[first]!r}")
