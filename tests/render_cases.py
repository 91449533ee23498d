"""The ray caster's edge cases and the rule its pictures are held to (tests/test_render_cases_cpu.py, tests/test_gpu_render_cases.py).

One authored scene: the pick-up scene, included, plus one world box, two world capsules and the cameras below.  A CASE is a
camera, an image size and a batch size; the batch cycles through three poses (joint positions and a cube placement), so the
numpy restatement (oracle/rcs_render_oracle.py) is evaluated for at most three frames per case and compared against every
environment.

The rule.  The restatement is evaluated at each pixel's centre and at the four points (+-delta, 0), (0, +-delta) beside it.  A
pixel is SETTLED when the five agree on hit or miss, on the shape entered first and on the entry face, and when their depths
differ by no more than a smooth surface allows: 4 x delta x the restatement's own depth gradient at the pixel.  Everything else
is GRAZING.  A picture under test has to equal the restatement at the centre on every settled pixel, and at the centre or at
one of the four offsets on a grazing one: either side of an edge, no third answer.  "Equal": the same hit or miss, raw depth
within `tol_gl`, colour within one level per channel.  One edge is not geometry: the floor's checker.  A settled pixel whose
five evaluations fall on different squares (CHECKER EDGE) is held to the centre in hit and depth like any settled pixel, and
its colour to one of the five: either square's, nothing else.  (Such pixels are no silhouette and are not counted as grazing:
a wide view of the floor crosses a few squares per pixel, and one pixel in a hundred then lies within 1e-3 pixel of an edge.)

delta is a condition of the test, not a measurement:
  * DELTA_F64 = 1e-9 pixel for the double-precision instantiation: its round-off is about 1e-16 of a metre-sized quantity and a
    pixel subtends more than 1e-3 rad, so two correct evaluations part at most ~1e-13 pixel from an edge;
  * DELTA_F32 = 1e-3 pixel for the product's float32 rays: a float32 ray direction and a float32 outline row are each good to
    about 1e-7 rad against pixels of 1e-2 to 1e-3 rad, i.e. 1e-5 to 1e-4 pixel -- more than an order of magnitude to spare.
The share of grazing pixels is capped ON THE RESTATEMENT ALONE (the CPU test): 0.5 % of a case's pixels at DELTA_F32,
0.01 % at DELTA_F64, so that nothing passes by excusing everything.  One pixel is undecided BY CONSTRUCTION and stands outside
the cap: the centre pixel of "down_face", whose ray runs exactly in the plane of a box face (DESIGNED_GRAZING).

tol_gl, the raw depth's tolerance.  Float64: one float32 ulp at 1.0 (2^-24): only the final rounding to float32 can differ.
Float32: measured on the restatement itself -- dtype=float32 against dtype=float64 over the settled pixels of every case,
written as (a + b znear / z) 2^-24 (the error of 1 / z enters the encoding scaled by znear / z) -- with a factor 4 on a and b
for what the kernel does differently (outline rows, m = n / (d - n . o), 1-ulp rcp and rsq).  A case in which that tolerance
would allow more than a millimetre at some pixel says nothing in float32 and is compared in float64 only (F64_ONLY): with
znear = 0.01 m the float32 depth buffer itself resolves a millimetre only out to a few metres.
"""

from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "robot-control-stack_amd")
for _p in (PKG, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rcs_render_oracle as RO  # noqa: E402

PICKUP_SCENE = os.path.join(PKG, "rcs_amd", "scenes", "fr3_simple_pick_up", "scene.xml")

DELTA_F64 = 1e-9
DELTA_F32 = 1e-3
CAP_F64 = 1e-4   # grazing pixels / pixels of a case, on the restatement alone
CAP_F32 = 5e-3
ULP = 2.0 ** -24
# Measured by `python tests/render_cases.py` (the largest |depth_gl(float32) - depth_gl(float64)| of the restatement over the
# pixels settled at DELTA_F32, all cases): a = the largest error in units of 2^-24 among pixels with znear / z < 0.02, b = the
# largest (error / 2^-24 - a) z / znear among the others.  Measured a = 5.000, b = 17.755 (profiles/render_cases/tests.txt).
A_MEASURED, B_MEASURED = 5.0, 17.76
TOL_FACTOR = 4.0
FAR_X = 0.02
# cases whose float32 tolerance would allow more than 1 mm somewhere (the floor towards the horizon, metres away): float64 only;
# "far_sky" is the same view in the scene variant with znear 0.02 m, in which a and b were not measured
F64_ONLY = ("level", "far_sky")
DESIGNED_GRAZING = {"down_face": ((15, 16),)}  # (row, column) of pixels whose ray lies exactly on an edge: what the case is for

# the world shapes added to the pick-up scene (binary fractions: the straight-down cameras' exact zeros depend on it)
# (and centres off the floor's checker lines, which a camera straight above them would otherwise look at through its centre column)
BOX_POS, BOX_HALF = (-0.5625, 0.5625, 0.125), (0.125, 0.0625, 0.125)
CAP_A_POS, CAP_A_R, CAP_A_HL = (-0.5625, -0.4375, 0.25), 0.0625, 0.125      # upright
CAP_B_FROM, CAP_B_TO, CAP_B_R = (-0.40, -0.75, 0.25), (-0.10, -0.75, 0.35), 0.07  # lying, tilted
N_SHAPES = 27  # floor, 11 hulls, the wrist camera's capsule, 10 finger pads, the cube; + 1 box + 2 capsules (kMaxShapes = 32)

Q_HOME = np.array([0.0, -np.pi / 4, 0.0, -3 * np.pi / 4, 0.0, np.pi / 2, np.pi / 4])
_rng = np.random.default_rng(20)
POSE_Q = Q_HOME + _rng.uniform(-0.4, 0.4, (3, 7))
# (the cube 0.1 mm into the floor, not at its half height 0.0288: exactly touching, round-off decides whether the first substep has a contact)
POSE_BOX = np.array([[0.50, 0.03, 0.0287, np.cos(0.35), 0, 0, np.sin(0.35)],
                     [0.43, -0.08, 0.0287, np.cos(-0.2), 0, 0, np.sin(-0.2)],
                     [0.56, 0.09, 0.0287, 1.0, 0, 0, 0]])


def _tilted(rx, ry, pos):
    qx = np.array([np.cos(rx / 2), np.sin(rx / 2), 0, 0])
    qy = np.array([np.cos(ry / 2), 0, np.sin(ry / 2), 0])
    w1, x1, y1, z1 = qx
    w2, x2, y2, z2 = qy
    q = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    return np.array([*pos, *q])


# the cube held in the air, tilted about x and y (the frame is taken two substeps later: it has fallen 0.1 mm)
POSE_BOX_TILTED = np.array([_tilted(0.5, 0.3, (0.5, 0.03, 0.2)), _tilted(-0.7, 0.4, (0.43, -0.08, 0.25)), _tilted(0.2, -0.9, (0.56, 0.09, 0.15))])


@dataclass(frozen=True)
class Case:
    name: str
    cam: str
    W: int
    H: int
    n_envs: int
    tilted: bool = False
    far: bool = False  # in the scene variant with twice the extent: znear 0.02 m, zfar 100 m


CASES = (
    # image and batch layouts: an existing camera, the three poses
    Case("1x1", "bird_eye_cam", 1, 1, 1),        # the smallest image, odd W: a lane's second ray outside the image
    Case("16x16", "bird_eye_cam", 16, 16, 8),    # exactly one tile; 8 workgroups: a multiple of 8
    Case("17x9", "bird_eye_cam", 17, 9, 1),      # odd W, H < 16: the second pass partly outside; 1 workgroup
    Case("33x31", "bird_eye_cam", 33, 31, 3),    # 6 tiles in one workgroup: tile >= ntile; 3 workgroups
    Case("50x40", "bird_eye_cam", 50, 40, 9),    # 12 tiles: each environment's second workgroup half empty; 18 workgroups
    Case("64x48", "bird_eye_cam", 64, 48, 5),    # the existing size at a batch that is no multiple of 8; 10 workgroups
    Case("64x48_wrist", "wrist_0", 64, 48, 5),
    # cameras, 33 x 31: an odd row and an odd column through the centre
    Case("level", "rc_level", 33, 31, 3),
    Case("under", "rc_under", 33, 31, 3),
    Case("down_box", "rc_down_box", 33, 31, 3),
    Case("down_face", "rc_down_face", 33, 31, 3),
    Case("capsule_axis", "rc_capsule_axis", 33, 31, 3),
    Case("capsule_side", "rc_capsule_side", 33, 31, 3),
    Case("near_box", "rc_near_box", 33, 31, 3),
    Case("near_hull", "rc_near_hull", 33, 31, 3),
    Case("inside_box", "rc_inside_box", 33, 31, 3),
    Case("inside_hull", "rc_inside_hull", 33, 31, 3),
    Case("fovy5", "rc_fovy5", 33, 31, 3),
    Case("fovy120", "rc_fovy120", 33, 31, 3),
    Case("border", "rc_border", 33, 31, 3),
    Case("tilted_cube", "rc_cube", 33, 31, 3, tilted=True),
    # the level camera with the far plane at 100 m: the sky's millimetre value does not fit uint16
    Case("far_sky", "rc_level", 33, 31, 3, far=True),
)
CASE_BY_NAME = {c.name: c for c in CASES}


def wgs_per_env(W, H):
    """render_wgs_per_env (csrc/render.h), restated: 16 x 16 tiles, two per wavefront, four wavefronts per workgroup."""
    return (((W + 15) // 16) * ((H + 15) // 16) + 7) // 8


# ---------------------------------------------------------------------------------------------------------------- the scene
def _look(pos, forward, up=(0.0, 0.0, 1.0), fovy=45.0):
    """A camera at `pos` looking along `forward` (the camera frame looks down -z, +y up): (pos, xyaxes, fovy)."""
    f = np.asarray(forward, dtype=np.float64)
    f = f / np.linalg.norm(f)
    x = np.cross(f, np.asarray(up, dtype=np.float64))
    x = x / np.linalg.norm(x)
    y = np.cross(x, f)
    return np.asarray(pos, dtype=np.float64), np.concatenate([x, y]), fovy


def _hull_entry(rs, g, origin, direction):
    """Where the ray enters hull g (shape frame = world for a world hull at the origin): (point, outward normal)."""
    pl = rs.planes[rs.plane_adr[g]: rs.plane_adr[g] + rs.plane_num[g]]
    nd, no = pl[:, :3] @ direction, pl[:, 3] - pl[:, :3] @ origin
    t = np.where(nd < 0, no / np.where(nd == 0, 1.0, nd), -np.inf)
    k = int(np.argmax(t))
    return origin + t[k] * direction, pl[k, :3] / np.linalg.norm(pl[k, :3])


def _world_pose(rs, g):
    assert rs.link[g] == -1
    return rs.rot[g].reshape(3, 3), rs.pos[g]


def hull_views_visible(rs, frames, cam, g):
    """k_hull_views' whole-image cull of shape g's bounding sphere, restated in float64."""
    link, cpos, crot, fovy, W, H = cam
    cR, cp = frames[link][0] @ np.asarray(crot).reshape(3, 3), frames[link][0] @ np.asarray(cpos) + frames[link][1]
    Rg, pg = frames[int(rs.link[g])]
    c = Rg @ (rs.rot[g].reshape(3, 3) @ rs.sphere[g][:3] + rs.pos[g]) + pg
    x, y, z = cR.T @ (c - cp)
    r = rs.sphere[g][3]
    ty = np.tan(fovy * np.pi / 360.0)
    tx = ty * W / H
    sides = ((x - tx * z, tx), (-x - tx * z, tx), (y - ty * z, ty), (-y - ty * z, ty))
    return bool(-z + r >= rs.znear and all(s >= 0 or s * s <= r * r * (1 + t * t) for s, t in sides))


def tile_visible(rs, frames, cam, g, c0, r0):
    """k_render_depth's cull of the same sphere against the pyramid of the 16 x 16 tile at (c0, r0), restated in float64."""
    link, cpos, crot, fovy, W, H = cam
    cR, cp = frames[link][0] @ np.asarray(crot).reshape(3, 3), frames[link][0] @ np.asarray(cpos) + frames[link][1]
    Rg, pg = frames[int(rs.link[g])]
    c = Rg @ (rs.rot[g].reshape(3, 3) @ rs.sphere[g][:3] + rs.pos[g]) + pg
    sx, sy, sz = cR.T @ (c - cp)
    r = rs.sphere[g][3]
    ty = np.tan(fovy * np.pi / 360.0)
    tx = ty * W / H
    xl, xr = (c0 * (2.0 / W) - 1) * tx, ((c0 + 16) * (2.0 / W) - 1) * tx
    yb, yt = (r0 * (2.0 / H) - 1) * ty, ((r0 + 16) * (2.0 / H) - 1) * ty
    sides = ((sx + xl * sz, xl), (-sx - xr * sz, xr), (sy + yb * sz, yb), (-sy - yt * sz, yt))
    return bool(-sz + r >= rs.znear and all(s >= 0 or s * s <= r * r * (1 + t * t) for s, t in sides))


def cull_disagreements(rs, frames, cam):
    """(hull, tile) pairs that the whole-image cull drops and the tile's own cull lets through."""
    _, _, _, _, W, H = cam
    out = []
    for g in range(len(rs.shape)):
        if rs.shape[g] != RO.SHAPE_HULL or hull_views_visible(rs, frames, cam, g):
            continue
        for r0 in range(0, H, 16):
            for c0 in range(0, W, 16):
                if tile_visible(rs, frames, cam, g, c0, r0):
                    out.append((g, c0, r0))
    return out


def _border_camera(rs, frames_by_pose):
    """Directed search over the yaw of a camera beside the robot for a placement in which, in every pose, some arm link's bounding
    sphere touches the image only beyond its border: a 33-pixel-wide image's last tile column reaches 15 pixels past the right edge,
    so the tile's pyramid still holds a sphere that the image's pyramid has lost.  Returns (pos, xyaxes, fovy) or None."""
    pos = np.array([1.3, 0.0, 1.1])
    for yaw in np.linspace(0.0, 1.2, 241):
        fwd = np.array([-np.cos(yaw), -np.sin(yaw), -1.0])  # (turning away from +y: the robot leaves through the right edge)
        p, xy, fovy = _look(pos, fwd)
        x, y = xy[:3], xy[3:]
        rot = np.stack([x, y, np.cross(x, y)], axis=1).reshape(9)
        cam = (-1, p, rot, fovy, 33, 31)
        if all(any(int(rs.link[g]) >= 0 for g, _, _ in cull_disagreements(rs, fr, cam)) for fr in frames_by_pose):
            # (the middle of a run of such yaws would be safer still; one grid step of 5 mrad against spheres of 0.1 m is margin enough)
            return p, xy, fovy
    return None


def _scene_xml(cameras, far=False):
    f = lambda v: " ".join(repr(float(x)) for x in v)  # noqa: E731
    cams = "\n".join(f'    <camera name="{n}" pos="{f(p)}" xyaxes="{f(xy)}" fovy="{fovy!r}"/>' for n, (p, xy, fovy) in cameras.items())
    # (the added world section comes first: the compiler wants the free cube's body and geom last in the file)
    return f"""<mujoco model="render_cases">
  <worldbody>
    <geom name="rc_box" type="box" pos="{f(BOX_POS)}" size="{f(BOX_HALF)}" rgba="0.8 0.3 0.2 1" contype="0" conaffinity="0"/>
    <geom name="rc_capsule_a" type="capsule" pos="{f(CAP_A_POS)}" size="{CAP_A_R!r} {CAP_A_HL!r}" rgba="0.2 0.3 0.9 1" contype="0" conaffinity="0"/>
    <geom name="rc_capsule_b" type="capsule" fromto="{f(CAP_B_FROM + CAP_B_TO)}" size="{CAP_B_R!r}" rgba="0.9 0.8 0.1 1" contype="0" conaffinity="0"/>
{cams}
  </worldbody>
  <include file="{PICKUP_SCENE}"/>{'<statistic extent="2"/>' if far else ''}
</mujoco>
"""


def _oracle_frames(cm, tilted):
    import rcs_oracle as O

    arm = [f"fr3_joint{i}_0" for i in range(1, 8)]
    out = []
    for k in range(3):
        o = O.Sim(cm, arm, arm, "attachment_site_0", "base_0", Q_HOME, None, "finger_joint1_0", "actuator8_0")
        o.reset(); o.robot_reset()
        o.box_qpos = (POSE_BOX_TILTED if tilted else POSE_BOX)[k]
        o.set_joints_hard(POSE_Q[k])
        o.step(2)
        out.append(RO.oracle_frames(o, cm))
    return out


@dataclass
class Scene:
    path: str
    cm: object
    rs: object
    frames: list         # per pose
    frames_tilted: list
    dropped: tuple       # cases that could not be built, with the reason
    far: object = None   # the same scene with <statistic extent="2"/> behind the include (the compiler takes the last one)

    def of(self, case):
        return self.far if case.far else self

    def cam(self, case):
        from rcs_amd import render

        return (*render.camera_in_link(self.cm, case.cam), case.W, case.H)

    def case_frames(self, case):
        return self.frames_tilted if case.tilted else self.frames


_SCENES: dict = {}


def build_scene(directory) -> Scene:
    """Write the cases' MJCF into `directory` and compile it; the cameras that depend on the hulls (next to one, inside one, a
    link at the image's border) are placed on a first compilation without them."""
    directory = str(directory)
    if directory in _SCENES:
        return _SCENES[directory]
    from rcs_amd import render
    from rcs_amd.mjcf import compile_mjcf

    bx, by, bz = BOX_POS
    hx, hy, hz = BOX_HALF
    cams = {
        # 0.3 m above the floor, level, looking at the robot along -x: sky above the horizon, the floor running to it
        "rc_level": (np.array([1.487, 0.013, 0.3]), np.array([0.0, 1, 0, 0, 0, 1]), 45.0),
        # under the floor, looking up: the plane is one-sided
        "rc_under": (np.array([0.3, 0.0, -0.5]), np.array([1.0, 0, 0, 0, -1, 0]), 45.0),
        # straight down, axes along the world's, exactly above the world box's centre / above its +x face's plane
        "rc_down_box": (np.array([bx, by, 1.0]), np.array([1.0, 0, 0, 0, 1, 0]), 45.0),
        # (the second rolled about its axis: the CENTRE ray alone runs in the face's plane, not a whole column of rays)
        "rc_down_face": (np.array([bx + hx, by, 1.0]), np.array([np.cos(0.3), np.sin(0.3), 0, -np.sin(0.3), np.cos(0.3), 0]), 45.0),
        # along the upright capsule's axis, centred on it; and the lying one from the side: wall and both caps
        "rc_capsule_axis": (np.array([CAP_A_POS[0], CAP_A_POS[1], 1.0]), np.array([1.0, 0, 0, 0, 1, 0]), 45.0),
        "rc_capsule_side": _look((-0.25, -1.2, 0.75), (0.0, 0.6, -0.6)),
        # 5 mm off the world box's +x face, looking along it at 60 degrees from its normal: the near plane cuts the face
        "rc_near_box": _look((bx + hx + 0.005, by, 0.15), (-0.5, np.sqrt(0.75), -1.2)),
        # inside the world box, looking at the robot
        "rc_inside_box": _look((bx, by, bz), (0.5, -0.5, 0.45)),
        # the cube, held in the air, from half a metre
        "rc_cube": _look((0.487, -0.45, 0.6), (0.013, 0.45, -0.4), fovy=20.0),
        "rc_fovy5": (np.array([0.271, -0.000, 2.080]), np.array([0.001, -1.000, -0.000, 1.000, 0.001, 0.017]), 5.0),
        "rc_fovy120": (np.array([0.271, -0.000, 2.080]), np.array([0.001, -1.000, -0.000, 1.000, 0.001, 0.017]), 120.0),
    }
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "render_cases.xml")
    with open(path, "w") as fh:
        fh.write(_scene_xml(cams))
    cm = compile_mjcf(path)
    rs = render.build_render_scene(cm, directory)
    g0 = rs.names.index("fr3_link0_collision_0")
    R0, p0 = _world_pose(rs, g0)
    assert np.array_equal(R0, np.eye(3)) and not p0.any()
    centre = rs.sphere[g0][:3].copy()
    pl0 = rs.planes[rs.plane_adr[g0]: rs.plane_adr[g0] + rs.plane_num[g0]]
    assert (pl0[:, :3] @ centre < pl0[:, 3]).all()  # inside the hull
    cams["rc_inside_hull"] = _look(centre, (0.4, 0.1, 1.0))
    hit, n = _hull_entry(rs, g0, centre + np.array([1.0, 0.3, 0.4]), -np.array([1.0, 0.3, 0.4]) / np.linalg.norm([1.0, 0.3, 0.4]))
    s = np.cross(n, [0.0, 0.0, 1.0])
    cams["rc_near_hull"] = _look(hit + 0.005 * n, -0.5 * n + np.sqrt(0.75) * s / np.linalg.norm(s) - np.array([0, 0, 1.2]))
    dropped = []
    border = _border_camera(rs, _oracle_frames(cm, False))
    if border is None:
        dropped.append(("border", "no yaw of the search puts a link's sphere between the image's and a tile's pyramid"))
    else:
        cams["rc_border"] = border
    with open(path, "w") as fh:
        fh.write(_scene_xml(cams))
    cm = compile_mjcf(path)
    rs = render.build_render_scene(cm, directory)
    assert len(rs.shape) == N_SHAPES <= 32, len(rs.shape)
    sc = Scene(path=path, cm=cm, rs=rs, frames=_oracle_frames(cm, False), frames_tilted=_oracle_frames(cm, True), dropped=tuple(dropped))
    far_path = os.path.join(directory, "render_cases_far.xml")
    with open(far_path, "w") as fh:
        fh.write(_scene_xml(cams, far=True))
    far_cm = compile_mjcf(far_path)
    far_rs = render.build_render_scene(far_cm, directory)
    assert far_rs.zfar == 2 * rs.zfar and far_rs.znear == 2 * rs.znear and 1000 * far_rs.zfar > 65535
    sc.far = Scene(path=far_path, cm=far_cm, rs=far_rs, frames=sc.frames, frames_tilted=sc.frames_tilted, dropped=())
    _SCENES[directory] = sc
    return sc


def active_cases(sc):
    gone = {n for n, _ in sc.dropped}
    return [c for c in CASES if c.name not in gone]


def near_cases(sc):
    """The cases of the scene as it is (znear 0.01 m): those the float32 tolerance is measured on."""
    return [c for c in active_cases(sc) if not c.far]


# ------------------------------------------------------------------------------------------------------------ the reference
def depth_gradient(rs, frames, cam, det):
    """|dz/dx| + |dz/dy| per pixel of the surface the restatement hit, from its own normal: a surface through the hit point with
    normal n is met by the ray of direction d at z = n . (q - o) / n . d, so dz = -z (n . dd) / (n . d)."""
    link, cpos, crot, fovy, W, H = cam
    cR = frames[link][0] @ np.asarray(crot).reshape(3, 3)
    ty = np.tan(fovy * np.pi / 360.0)
    ddx, ddy = cR[:, 0] * (2.0 * ty / H), cR[:, 1] * (2.0 * ty / H)  # (tx 2 / W = ty 2 / H)
    nw = np.zeros(det["normal"].shape)
    for g in np.unique(det["shape"][det["hit"]]):
        R = frames[int(rs.link[g])][0] @ rs.rot[g].reshape(3, 3)
        nw = np.where((det["shape"] == g)[..., None], det["normal"] @ R.T, nw)
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = det["z"] * (np.abs(nw @ ddx) + np.abs(nw @ ddy)) / np.abs((nw * det["ray"]).sum(-1))
    return np.where(det["hit"], np.nan_to_num(grad, nan=np.inf), 0.0)


def settled_mask(rs, frames, cam, centre, beside, delta):
    ok = np.ones(centre["hit"].shape, dtype=bool)
    bound = 4.0 * delta * depth_gradient(rs, frames, cam, centre) + 64 * np.finfo(np.float64).eps * centre["z"]
    for o in beside:
        ok &= (o["hit"] == centre["hit"]) & (o["shape"] == centre["shape"]) & (o["face"] == centre["face"])
        ok &= ~centre["hit"] | (np.abs(o["z"] - centre["z"]) <= bound)
    return ok


_OFFSETS = ((1, 0), (-1, 0), (0, 1), (0, -1))


@functools.lru_cache(maxsize=None)
def _reference(directory, name):
    case = CASE_BY_NAME[name]
    sc = build_scene(directory).of(case)
    cam = sc.cam(case)
    return [frame_reference(sc.rs, cam, fr) for fr in sc.case_frames(case)[: min(3, case.n_envs)]]


def frame_reference(rs, cam, fr, keys=("f64", "f32")):
    """One frame's reference: the restatement at the pixel centres and beside them, and which pixels that settles."""
    centre = RO.render_depth(rs, cam, fr, detail=True)
    ref = {"centre": centre}
    for key in keys:
        delta = {"f64": DELTA_F64, "f32": DELTA_F32}[key]
        beside = [RO.render_depth(rs, cam, fr, offset=(dx * delta, dy * delta), detail=True) for dx, dy in _OFFSETS]
        ref[key] = {"beside": beside, "settled": settled_mask(rs, fr, cam, centre, beside, delta),
                    "checker_edge": np.any([o["checker"] != centre["checker"] for o in beside], axis=0)}
    return ref


def reference(sc, case):
    """Per pose of the case: {"centre": detail, "f64" / "f32": {"beside": [4 details], "settled": mask, "checker_edge": mask}} (computed once)."""
    return _reference(sc.path.rsplit(os.sep, 1)[0], case.name)


def tol_gl(z, znear, double_precision):
    if double_precision:
        return np.full(np.shape(z), ULP)
    return TOL_FACTOR * (A_MEASURED + B_MEASURED * znear / z) * ULP


def tolerance_in_metres(z, znear, zfar):
    """What the float32 tol_gl allows in view depth at depth z: dz = tol / (d depth_gl / dz), depth_gl = (1/near - 1/z) / (1/near - 1/far)."""
    return tol_gl(z, znear, False) * z * z * (1.0 / znear - 1.0 / zfar)


def host_mm(raw, znear, zfar):
    """python/rcs/camera/sim.py:57-86 on a raw depth buffer [.., H, W] rows bottom-up: millimetres [.., H, W] uint16 rows top-down."""
    frame = raw[..., ::-1, :]
    with np.errstate(invalid="ignore"):
        z = np.float32(znear) / (np.float32(1) - frame * np.float32(1 - znear / zfar))
        return (z * np.float32(1000)).astype(np.uint16)


def fits_uint16(raw, znear, zfar):
    """Pixels (rows top-down, as host_mm) whose millimetre value is below 65536: numpy's cast of anything else is not defined."""
    frame = raw[..., ::-1, :].astype(np.float64)
    return 1000.0 * znear / (1 - frame * (1 - znear / zfar)) < 65535.0


# ----------------------------------------------------------------------------------------------------------- the comparison
def _equal(raw, rgb, cand, znear, double_precision):
    """Per pixel: does the picture equal this evaluation of the restatement -- in hit and depth, in colour?  (and the raw depth's
    deviation from it)"""
    dev = np.abs(raw.astype(np.float64) - cand["depth_gl"].astype(np.float64))
    ok = ((raw < 1.0) == (cand["depth_gl"] < 1.0)) & (dev <= tol_gl(cand["z"], znear, double_precision))
    same_colour = np.ones(ok.shape, dtype=bool) if rgb is None else np.abs(rgb.astype(np.int64) - cand["rgb"].astype(np.int64)).max(axis=-1) <= 1
    return ok, same_colour, dev


def compare(sc, case, raw, rgb, double_precision, refs=None):
    """raw [n, H, W] float32 and rgb [n, H, W, 3] uint8 (or None), rows bottom-up, against the case's reference: the report."""
    return compare_frames(sc.of(case).rs, reference(sc, case) if refs is None else refs, raw, rgb, double_precision, case.name)


def compare_frames(rs, refs, raw, rgb, double_precision, name="", rep=None):
    """Frame e of raw / rgb against refs[e % len(refs)] (frame_reference); `rep`: a report to add to."""
    key = "f64" if double_precision else "f32"
    rep = rep if rep is not None else {"case": name, "pixels": 0, "grazing": 0, "checker_edge": 0, "unexcused": 0, "first_unexcused": [], "max_settled_dev": 0.0, "max_settled_tol": 0.0}
    for e in range(raw.shape[0]):
        ref = refs[e % len(refs)]
        settled = ref[key]["settled"]
        rgb_e = None if rgb is None else rgb[e]
        depth_c, colour_c, dev = _equal(raw[e], rgb_e, ref["centre"], rs.znear, double_precision)
        ok_any, colour_any = depth_c & colour_c, colour_c.copy()
        for o in ref[key]["beside"]:
            depth_o, colour_o, _ = _equal(raw[e], rgb_e, o, rs.znear, double_precision)
            ok_any |= depth_o & colour_o
            colour_any |= colour_o
        edge = settled & ref[key]["checker_edge"]
        bad = np.where(settled, ~(depth_c & np.where(edge, colour_any, colour_c)), ~ok_any)
        rep["pixels"] += bad.size
        rep["grazing"] += int((~settled).sum())
        rep["checker_edge"] += int(edge.sum())
        rep["unexcused"] += int(bad.sum())
        both = settled & (raw[e] < 1.0) & ref["centre"]["hit"]
        if both.any():
            k = int(np.argmax(np.where(both, dev, -1.0)))
            if dev.flat[k] > rep["max_settled_dev"]:
                rep["max_settled_dev"] = float(dev.flat[k])
                rep["max_settled_tol"] = float(tol_gl(ref["centre"]["z"], rs.znear, double_precision).flat[k])
        for r, c in zip(*np.nonzero(bad)):
            if len(rep["first_unexcused"]) < 5:
                rep["first_unexcused"].append(dict(
                    env=e, row=int(r), col=int(c), settled=bool(settled[r, c]), kernel=(float(raw[e, r, c]), None if rgb is None else rgb[e, r, c].tolist()),
                    reference=[(float(o["depth_gl"][r, c]), o["rgb"][r, c].tolist(), int(o["shape"][r, c]), int(o["face"][r, c]))
                               for o in (ref["centre"], *ref[key]["beside"])]))
    return rep


def summary(rep):
    return (f"{rep['case']:>13}  pixels {rep['pixels']:6d}  grazing {rep['grazing']:4d}  checker edge {rep['checker_edge']:4d}  unexcused {rep['unexcused']:4d}  "
            f"max dev settled {rep['max_settled_dev'] / ULP:7.3f} ulp (tol_gl there {rep['max_settled_tol'] / ULP:7.3f} ulp)")


# ---------------------------------------------------------------------------------------------------------- the GPU's side
def render_on_gpu(sc, case, double_precision):
    """The case through the product's calls: (raw [n,H,W] of render_raw_rgbd, rgb [n,H,W,3], raw of the depth-only render_raw,
    fused millimetres of render_depth_mm, the host layer's millimetres and colour of get_latest_frames)."""
    from rcs_amd import sim as S
    from rcs_amd.camera import SimCameraConfig, SimCameraSet
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    n = case.n_envs
    sc = sc.of(case)
    cfg = default_sim_robot_cfg("fr3_simple_pick_up")
    simu = S.Sim(sc.path, S.SimConfig(), n_envs=n)
    try:
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
        cs = SimCameraSet(simu, {"c": SimCameraConfig(identifier=case.cam, frame_rate=0, resolution_width=case.W, resolution_height=case.H)},
                          physical_units=True, render_on_demand=True)
        cs.set_double_precision(double_precision)
        assert len(cs._scene.shape) == N_SHAPES
        simu.reset(); robot.reset()
        idx = np.arange(n) % 3
        simu.set_free_joint_qpos("box_joint", (POSE_BOX_TILTED if case.tilted else POSE_BOX)[idx])
        robot.set_joints_hard(POSE_Q[idx])
        simu.step(2)
        rgb, raw, _, _ = cs.render_raw_rgbd("c")
        raw_depth_only, _, _ = cs.render_raw("c")
        fused = cs.render_depth_mm("c")
        fr = cs.get_latest_frames().frames["c"].camera
        return dict(raw=raw, rgb=rgb, raw_depth_only=raw_depth_only, fused=fused, frames_mm=fr.depth.data[..., 0], frames_rgb=fr.color.data)
    finally:
        simu.close()


# ------------------------------------------------------------------------------------------- the float32 tolerance, measured
def measure_f32(sc, cases=None):
    """Per case: (a, b, what the resulting tolerance allows in metres at its worst pixel, settled pixels) of the restatement in
    float32 against itself in float64 on the pixels settled at DELTA_F32; a, b as described at A_MEASURED."""
    rows = {}
    for case in (near_cases(sc) if cases is None else cases):
        assert not case.far  # (a and b are measured in the scene they are used in: znear 0.01 m)
        cam = sc.cam(case)
        x, err, z = [], [], []
        for fr, ref in zip(sc.case_frames(case), reference(sc, case)):
            d32 = RO.render_depth(sc.rs, cam, fr, dtype=np.float32)[0]
            m = ref["f32"]["settled"] & ref["centre"]["hit"] & (d32 < 1.0)
            err.append(np.abs(d32.astype(np.float64) - ref["centre"]["depth_gl"].astype(np.float64))[m] / ULP)
            z.append(ref["centre"]["z"][m])
        err, z = np.concatenate(err), np.concatenate(z)
        x = sc.rs.znear / z
        rows[case.name] = dict(err=err, x=x, z=z)
    far = np.concatenate([r["err"][r["x"] < FAR_X] for r in rows.values()])
    a = float(far.max())
    b = max(float(((r["err"] - a) / r["x"])[r["x"] >= FAR_X].max(initial=0.0)) for r in rows.values())
    out = {"a": a, "b": max(b, 0.0), "cases": {}}
    for name, r in rows.items():
        worst = float(tolerance_in_metres(r["z"], sc.rs.znear, sc.rs.zfar).max(initial=0.0))
        out["cases"][name] = dict(settled_hit_pixels=int(r["err"].size), max_err_ulp=float(r["err"].max(initial=0.0)), z_min=float(r["z"].min(initial=np.inf)),
                                  z_max=float(r["z"].max(initial=0.0)), allows_m=worst)
    return out


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        sc = build_scene(tmp)
        print("dropped:", sc.dropped)
        res = measure_f32(sc)
        print(f"measured a = {res['a']:.3f}  b = {res['b']:.3f}  (units of 2^-24; tolerance = {TOL_FACTOR:g} x (a + b znear / z) 2^-24 with the constants in this file)")
        for name, r in res["cases"].items():
            ref = reference(sc, CASE_BY_NAME[name])
            px = sum(x["centre"]["hit"].size for x in ref)
            print(f"{name:>13}  pixels {px:5d}  grazing f32 {sum(int((~x['f32']['settled']).sum()) for x in ref):3d}  f64 {sum(int((~x['f64']['settled']).sum()) for x in ref):3d}"
                  f"  checker edge f32 {sum(int(x['f32']['checker_edge'].sum()) for x in ref):3d}  f64 {sum(int(x['f64']['checker_edge'].sum()) for x in ref):3d}"
                  f"  settled hits {r['settled_hit_pixels']:5d}  max err {r['max_err_ulp']:6.3f} ulp  z {r['z_min']:.4f}..{r['z_max']:.3f} m"
                  f"  float32 tol allows {1e3 * r['allows_m']:8.4f} mm{'  -> float64 only' if r['allows_m'] > 1e-3 else ''}")
