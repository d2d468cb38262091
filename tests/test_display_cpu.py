"""CPU: the displayed frame's exact rule (include/vxrt.h: VXRT_DISPLAY_BGRA8_SRGB / VXRT_DISPLAY_RGBA8_SRGB) — the threshold table the
library encodes with, the binary64 oracle the GPU tests compare against, and the C++ mirror's members for display read-back.

The oracle restates the rule with its specials written out: NaN, x <= 0 -> 0; x >= 1 -> 255; else round_half_up(255 * S(x)) with
S(x) = 12.92 x (x <= 0.0031308), 1.055 x^(1/2.4) - 0.055; alpha round_half_up(255 * clamp(a, 0, 1)), NaN -> 0.  In binary64 it is
correctly rounded for every binary32 input (no input comes within 2.2e-9 of a step of a half-step)."""
import os
import subprocess

import numpy as np

from conftest import ROOT

BGRA, RGBA = 5, 6


def colour_oracle(x):
    """float32 array -> uint8 colour bytes, the rule in binary64."""
    with np.errstate(invalid="ignore"):                 # signalling NaNs widen quietly
        x = np.asarray(x, np.float32).astype(np.float64)
    inside = (x > 0.0) & (x < 1.0)                      # NaN compares false
    v = np.where(inside, x, 0.5)
    s = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    byte = np.floor(255.0 * s + 0.5)
    return np.where(inside, byte, np.where(x >= 1.0, 255.0, 0.0)).astype(np.uint8)


def alpha_oracle(a):
    with np.errstate(invalid="ignore"):
        a = np.asarray(a, np.float32).astype(np.float64)
    inside = (a > 0.0) & (a < 1.0)
    byte = np.floor(np.where(inside, a, 0.0) * 255.0 + 0.5)
    return np.where(inside, byte, np.where(a >= 1.0, 255.0, 0.0)).astype(np.uint8)


def display_oracle(rgba, fmt):
    """float32 [..., 4] (r, g, b, a) -> uint8 [..., 4] in the byte order of `fmt` (BGRA = 5, RGBA = 6)."""
    rgba = np.asarray(rgba, np.float32)
    r, g, b = (colour_oracle(rgba[..., i]) for i in range(3))
    a = alpha_oracle(rgba[..., 3])
    return np.stack((b, g, r, a) if fmt == BGRA else (r, g, b, a), axis=-1)


def threshold_windows(t, ulps):
    """Every binary32 value within +-ulps bit patterns of each threshold (all thresholds are positive and below 1)."""
    bits = t.view(np.uint32).astype(np.int64)
    w = (bits[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]).reshape(-1)
    return w.astype(np.uint32).view(np.float32)


def test_thresholds_are_exactly_the_steps_of_the_rule(H):
    t = H.display_thresholds()
    assert t.dtype == np.float32 and t.shape == (255,)
    assert np.all(t > 0) and np.all(t < 1) and np.all(np.diff(t) > 0)
    at = colour_oracle(t).astype(int)
    below = colour_oracle(np.nextafter(t, np.float32(-np.inf))).astype(int)
    k = np.arange(255)
    assert np.all(at >= k + 1), np.nonzero(at < k + 1)
    assert np.all(below <= k), np.nonzero(below > k)
    # the byte of x is the number of thresholds <= x, on every value near a step
    x = threshold_windows(t, 4096)
    assert np.array_equal(colour_oracle(x), np.searchsorted(t, x, side="right").astype(np.uint8))
    L = H.lib()
    assert L.vxrt_display_thresholds(None) == H.E_INVALID


def test_the_oracle_is_frame_loop_srgb8_on_the_threshold_windows(H):
    from gpu_voxel_raytracer_amd import frame_loop
    x = threshold_windows(H.display_thresholds(), 4096)
    got = frame_loop.srgb8(x.reshape(-1, 3))                          # 2.09 M values, three per "pixel"
    assert np.array_equal(got.reshape(-1), colour_oracle(x))
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1.0, 2.0, 0.0031308, 1e-45, np.float32(1) - np.float32(2 ** -24)],
                       np.float32)
    assert np.array_equal(frame_loop.srgb8(special), colour_oracle(special))
    assert colour_oracle(np.float32(0.5)) == 188 and alpha_oracle(np.float32(1.0)) == 255 and alpha_oracle(np.float32(np.nan)) == 0


def test_byte_orders_of_the_oracle():
    px = np.array([[0.25, 0.5, 1.0, 1.0]], np.float32)
    r, g, b = (int(colour_oracle(v)) for v in px[0, :3])
    assert display_oracle(px, BGRA).tolist() == [[b, g, r, 255]]
    assert display_oracle(px, RGBA).tolist() == [[r, g, b, 255]]


def test_python_layer_knows_the_display_images(H):
    import gpu_voxel_raytracer_amd as pkg
    assert (pkg.DISPLAY_BGRA8_SRGB, pkg.DISPLAY_RGBA8_SRGB) == (5, 6) == (H.DISPLAY_BGRA8_SRGB, H.DISPLAY_RGBA8_SRGB)
    text = open(os.path.join(ROOT, "include", "vxrt.h")).read()
    assert "VXRT_DISPLAY_BGRA8_SRGB = 5" in text and "VXRT_DISPLAY_RGBA8_SRGB = 6" in text
    assert H.lib().vxrt_abi_version() == 6


CPP = r"""
#include <cstdio>
#include "vxrt.hpp"
#include "vxrt_debug.h"

// compiled and linked only: a context needs a GPU
[[maybe_unused]] static void display_loop(vxrt::Context& ctx) {
    std::vector<uint8_t> shown = ctx.read_display(VXRT_DISPLAY_RGBA8_SRGB);
    vxrt::PinnedDisplay slots[2] = {vxrt::PinnedDisplay(ctx.display_bytes()), vxrt::PinnedDisplay(ctx.display_bytes())};
    for (uint32_t f = 0; f < 4; f++) {
        ctx.render(VXRT_ALL);
        if (f >= 1) ctx.read_wait((f + 1) & 1);
        ctx.read_async(VXRT_DISPLAY_BGRA8_SRGB, slots[f & 1], f & 1);
    }
    ctx.read_wait(0);
    ctx.read_wait(1);
    std::printf("%zu %zu %u\n", shown.size(), slots[0].bytes(), unsigned(slots[1].data()[0]));
}

int main() {
    float t[255];
    if (vxrt_display_thresholds(t) != VXRT_OK) return 1;
    std::printf("%.9g %.9g\n", double(t[0]), double(t[254]));
    return 0;
}
"""


def test_cpp_mirror_has_display_read_back(H, tmp_path):
    from gpu_voxel_raytracer_amd import _build
    src = tmp_path / "display.cpp"
    src.write_text(CPP)
    exe = tmp_path / "display"
    libdir = os.path.dirname(_build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lvxrt", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    t = H.display_thresholds()
    assert [np.float32(v) for v in out.stdout.split()] == [t[0], t[254]]
