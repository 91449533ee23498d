"""The ray caster (csrc/render.h: k_shape_frames, k_hull_views, k_render_depth) against the numpy restatement pixel by pixel,
at the image and batch layouts and from the cameras of tests/render_cases.py, in both instantiations, depth and colour.

The rule (tests/render_cases.py): a pixel whose answer the restatement itself decides -- the same hit, shape and face at the
centre and 1e-9 (float64) / 1e-3 (float32) pixel beside it -- has to be the restatement's: raw depth within tol_gl, colour within
one level, never a hit for a miss; a grazing pixel has to be one of the restatement's five answers.  No pixel is excused by number.

Millimetres: the fused path (render_depth_mm) and the host layer (get_latest_frames) are both the conversion of the kernel's own raw
depth, bit for bit, on every pixel of every case.  With the scene's own clip planes (znear 0.01 m, zfar 50 m) every value fits uint16:
a ray that hits nothing has raw depth 1.0 and converts -- in float32, near / (1 - 1.0 * float32(1 - near / far)) * 1000 -- to 50006,
not to 50000.  The case "far_sky" doubles the extent (zfar 100 m): its sky converts to 100013.2 mm, which does not fit.  numpy's cast of
such a value is not defined, so the restatement's millimetres are not consulted there (render_cases.fits_uint16: raw depth only); what
IS asserted is that the fused path and the host layer write the same thing, and what it is: the low 16 bits of the truncated value, 34477.

Cases compared in float64 only: render_cases.F64_ONLY (there the measured float32 tolerance would allow more than a millimetre)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

SKY_MM = 50006      # zfar = 50 m
SKY_MM_FAR = 34477  # zfar = 100 m: float32 100013.2 -> 100013 -> its low 16 bits (what the host layer's numpy cast and the kernel's both write)


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    return RC.build_scene(tmp_path_factory.mktemp("render_cases"))


@pytest.mark.parametrize("double_precision", [False, True], ids=["float32", "float64"])
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_case_matches_the_reference_pixel_by_pixel(sc, name, double_precision):
    case = RC.CASE_BY_NAME[name]
    assert name not in {n for n, _ in sc.dropped}, sc.dropped
    try:
        k = RC.render_on_gpu(sc, case, double_precision)
    except Exception as ex:  # a call that failed on the device: nothing more is started on it
        pytest.exit(f"{name}: the device call failed: {ex!r}", returncode=3)
    n, H, W = case.n_envs, case.H, case.W
    assert k["raw"].shape == (n, H, W) and k["rgb"].shape == (n, H, W, 3) and k["fused"].shape == (n, H, W)
    # millimetres and the host layer's frames: conversions of the kernel's own raw depth, wherever the value fits uint16
    rs = sc.of(case).rs
    fits = RC.fits_uint16(k["raw"], rs.znear, rs.zfar)
    host = RC.host_mm(k["raw"], rs.znear, rs.zfar)
    sky = k["raw"][:, ::-1] == 1.0
    assert int((k["fused"] != host)[fits].sum()) == 0
    # the fused path against the host layer's conversion of the same buffer: on EVERY pixel, those beyond uint16 included
    assert int((k["fused"] != k["frames_mm"]).sum()) == 0, (np.unique(k["fused"][~fits]), np.unique(k["frames_mm"][~fits]))
    if case.far:
        assert (~fits).sum() > 100 and np.array_equal(~fits, sky)
        print("far_sky: the sky's millimetre value as written:", np.unique(k["fused"][sky]), "host layer:", np.unique(k["frames_mm"][sky]))
        assert (k["fused"][sky] == SKY_MM_FAR).all()
    else:
        assert fits.all() and (k["fused"][sky] == SKY_MM).all()
    assert np.array_equal(k["frames_rgb"], k["rgb"][:, ::-1])
    if not double_precision and name in RC.F64_ONLY:
        return  # (the raw depth says nothing there in float32: see render_cases.F64_ONLY)
    rep = RC.compare(sc, case, k["raw"], k["rgb"], double_precision)
    print(("float64" if double_precision else "float32"), RC.summary(rep))
    # the depth-only kernel (render_raw: another instantiation of the same template) under the same rule, without colour
    rep_d = RC.compare(sc, case, k["raw_depth_only"], None, double_precision)
    print("     depth only", RC.summary(rep_d))
    assert rep["unexcused"] == 0, rep
    assert rep_d["unexcused"] == 0, rep_d
